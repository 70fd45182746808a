"""The public HAVC entry points without VapourSynth, executed on the MI355X:

    HAVC_colorizer   vsdeoldify/__init__.py:2290-2523     HAVC_merge       vsdeoldify/__init__.py:2536-2675
    HAVC_ddeoldify   vsdeoldify/__init__.py:3612-3628     ddeoldify        vsdeoldify/__init__.py:3642-3653
    HAVC_stabilizer  vsdeoldify/__init__.py:2748-2873     HAVC_clip_slice / HAVC_clip_reconstruct (+ ClipTiles)  vsdeoldify/__init__.py:2886-2945
    HAVC_SceneDetect vsdeoldify/__init__.py:3191-3225     (-> scdetect.SceneInfo: arrays carry no frame props)
    HAVC_SceneDetectEdges vsdeoldify/__init__.py:3227-3258   (the edge-masked detector + its SSIM / histogram filter -> scdetect_edge.EdgeSceneInfo; scdetect_edge.py)
    HAVC_deepex      vsdeoldify/__init__.py:1421-1735     (ex_model 0 = ColorMNet, method 0; `scenes=` is the SceneInfo the reference reads off clip_ref's props)
    HAVC_bw_tune     vsdeoldify/__init__.py:1266-1339     HAVC_auto_levels vsdeoldify/__init__.py:3150-3179   (methods 0-3: CLAHE / equalizeHist; equalize.py)
    HAVC_DeepRemaster vsdeoldify/__init__.py:2689-2735    (mode 0: reference stills from a directory; remaster_render.RemasterRender; fast mode only)
    HAVC_extract_reference_frames vsdeoldify/__init__.py:3272-3351   (sc_algo 0: SceneDetect + the SSIM / histogram post-filter, then ref_nnnnnn.jpg|png on disk)
    HAVC_export_reference_frames  vsdeoldify/__init__.py:3364-3385   HAVC_export_list_frames vsdeoldify/__init__.py:3387-3416   (the writers alone)
    HAVC_recover_clip_color vsdeoldify/__init__.py:2956-2992   (ChromaRetentionMerge on a clip: gradient and binary mask, chroma_resize through the library's Spline64)
    HAVC_restore_video vsdeoldify/__init__.py:1959-2127   (colour transfer from a reference video: ex_model 0 = ColorMNet, 2 = DeepRemaster's clip mode; methods 5, 6)
    HAVC_retinex     vsdeoldify/__init__.py:1073-1101     (multi-scale Retinex, MSRCP, with the luma gate and blend of vs_retinex_fast; float64 Gaussians; retinex.py)
    HAVC_tweak       vsdeoldify/__init__.py:1377-1408     (hue, saturation, brightness, contrast, gamma through a YUV420P8 round trip; tweak.py)
    HAVC_adjust_rgb  vsdeoldify/__init__.py:1342-1374     (grey-world normalisation, per-channel gain, bias and gamma as per-frame tables; tweak.py)
    HAVC_rgb_denoise vsdeoldify/__init__.py:924-944       (rgb_balance + CLAHE on luma between the TV-range conversions: the equalize.py path)
    HAVC_TimeCube    vsdeoldify/__init__.py:2995-3026     (a 3D LUT from a .cube file, vs_tweak with the effect's factors, merge by strength; timecube.py)
    HAVC_clip_overlay vsdeoldify/__init__.py:3029-3148    (an overlay placed on a base: nine blend modes, mask, opacity, planes; overlay.py)

Same names, argument lists, defaults, parameter normalisation, frame-size rule, model routing, combine dispatch
(vsslib/mcomb.py:125-192) and error texts; a "clip" is a uint8 array [n, h, w, 3] (or one frame [h, w, 3], or a
`device.DeviceImage` of either shape: then the whole graph runs without leaving HBM).  `HAVCFrameColorizer` is the object
behind `HAVC_colorizer` (models and nets are built once and reused between calls).

What only VapourSynth can do stays there and is REFUSED here instead of being approximated: `vs_tweak` (deoldify / ddcolor
sat / hue other than 1 / 0, `luma_mask_sat` < 1), scene detection INSIDE HAVC_colorizer / HAVC_ddeoldify (`sc_threshold` > 0, `sc_min_freq` > 0: the reference-frame
logic of vs_sc_ddcolor / vs_sc_tweak that hangs off it), the SSIM post-filter INSIDE HAVC_SceneDetect (`sc_tht_ssim` in (0, 1), `sc_min_int` > 1: that refusal is pinned and
stays; the filter itself is built and runs in HAVC_extract_reference_frames), the plugin scene detectors of HAVC_extract_reference_frames (`sc_algo` 1-3; 1 is built as HAVC_SceneDetectEdges but not routed there yet), of HAVC_deepex the exemplar models 1-3 (Deep-Exemplar, DeepRemaster: not built), methods 1-6
(reference frames from a directory or a video), `encode_mode` 2 and `sc_framedir` / `only_ref_frames` (they write files), the parts of the DDColor
pre-tweaks that are VapourSynth filters (`ddtweak`: bright / cont / gamma through vs_tweak, rgb_denoise, retinex), non-RGB24 formats.
Computed here: the hue adjustment vs_sc_ddcolor applies to every DDColor frame (default "300:360|0.8,0.1") and the luma-constrained
pre-tweak with its luma recovery (HAVCFrameColorizer._read_ddtweak).  What stands in for VapourSynth native code (outside the parity
contract; none of it can be executed where the fixtures are made, so its integer rounding is unpinned):
  * zimg's `resize.Spline64` -> the library's own Spline64; zimg's `resize.Spline36` (HAVC_restore_video: clip_ref to the clip's size) -> the library's own
    Spline36, the same passes with the other kernel;
  * `std.MaskedMerge` under an `akarin.Expr` position mask (HAVC_clip_reconstruct's row and column blends, vsslib/vstiles4.py:281-349) ->
    out = (a * (255 - m) + b * m + 127) // 255 per channel, rounded to uint8 after each of the two blends; m = 0 gives a and m = 255 gives b exactly;
  * `vsresize.resize_to_chroma` (HAVC_clip_reconstruct(chroma_resize=True), vsslib/vsresize.py:101-127: a zimg YUV420P8 round trip, BT.709) -> the
    luma re-attach the rest of this file uses, vs_recover_clip_luma = chroma_post_process (cv2 BT.601 YUV, no chroma subsampling), with clip_orig as
    the luma source.
  * HAVC_SceneDetect (vsdeoldify_amd/scdetect.py has the details): zimg's RGB -> GRAY8 with matrix 709 -> Y = (cr * R + cg * G + cb * B + bias) >> 16, limited
    range by default (VapourSynth's default for non-RGB output; `luma_range="full"` exists because that assumption cannot be checked here); `resize_min_HW`'s zimg
    Spline36 on the gray plane -> the library's Spline64 on the RGB clip, at the reference's size; `misc.SCDetect` on the default path (threshold >= 0.10,
    offset 1) -> prev_n = diff(n - 1, n) > threshold, prev_0 = 1, next_n = prev_(n + 1), next_last = 1.  The custom detector (threshold < 0.10 or offset > 1) and
    the black / white filter are the reference's Python, restated and pinned by tests/golden/scdetect.npz.
  * HAVC_SceneDetectEdges (vsdeoldify_amd/scdetect_edge.py has the details): the gray conversion and resize as above; std.Convolution (Kirsch), akarin.Expr,
    TCanny(mode=1), std.MaskedMerge and std.PlaneStats -> the integer / float32 sequences of tests/scedges_util.py, which csrc/scedge.hip equals byte for
    byte; misc.SCDetect(threshold=0.10) -> the rule above on the SAD against the previous frame.  Both selectors are the reference's Python, restated and
    pinned by tests/golden/scdetect_edges.npz -- the missing comma of its prop list included.
  * the SSIM / histogram post-filter (HAVC_extract_reference_frames; scdetect.py has the details): skimage's structural_similarity -> its published formula
    over exact integer 7 x 7 window sums, float64 quotient; cv2's gray -> (4899 R + 9617 G + 1868 B + 8192) >> 14; cv2.calcHist -> exact counts;
    cv2.normalize + compareHist(HELLINGER) (float32 histograms there) -> OpenCV's published definition in float64; the zimg resize of the RGB clip in
    front of the filter -> the library's Spline64.  None of skimage, cv2 or zimg can be executed where the fixtures are made.  The selector on top of
    the two scores is the reference's Python, restated and pinned by tests/golden/scfilter.npz.
  * HAVC_bw_tune / HAVC_auto_levels (vsdeoldify_amd/equalize.py has the details): `std.Levels` -> a 256-entry table, `resize.Bicubic(range_in_s, range_s)` at
    unchanged size -> a per-sample range scale rounded to nearest (the reference applies both, on the way in and on the way out: so does this), `std.Merge` ->
    a + (((b - a) * w15 + 16384) >> 15), `std.PlaneStats` -> sum / (n_pixels * 255), `std.Expr "x g *"` -> a float32 product rounded half to even; cv2's CLAHE
    and equalizeHist follow OpenCV's published algorithm (cv2 cannot be executed there either).  The gate, the f_luma roundings, the blend weights, Pillow's
    blend and rgb_balance's gains are the reference's Python, restated and pinned by tests/golden/equalize.npz.  Methods 4 (timecube plugin + LUT files) and
    5 (Retinex MSRCP plugin) and `chroma_resize=True` (a zimg round trip inside convert_format_RGB24) are refused.
  * HAVC_retinex (vsdeoldify_amd/retinex.py has the details): the `retinex.MSRCP` plugin -> the published MSRCP algorithm (Petro / Sbert / Morel, IPOL 2014)
    with the Young - van Vliet recursive Gaussian, float64, restated in tests/retinex_util.py -- the plugin cannot be executed where the fixtures are made.
    The gate, the f_luma roundings, the blend weight, Pillow's blend and the arguments handed to the plugin are the reference's Python, restated and pinned
    by tests/golden/retinex.npz.  `chroma_resize=True` is refused; method 5 of HAVC_bw_tune / HAVC_auto_levels is not routed here yet and stays refused.
  * HAVC_tweak / HAVC_adjust_rgb / HAVC_rgb_denoise (vsdeoldify_amd/tweak.py has the details): zimg's `resize.Bicubic` RGB24 -> YUV420P8 -> RGB24 (BT.709,
    full range; Mitchell bicubic chroma resampling, `dither_type="error_diffusion"` on the way back), `std.Levels(gamma=)`, `std.Expr`, `std.Lut` -> the
    float32 sequences of tests/tweak_util.py, which csrc/tweak.hip equals byte for byte; none of it can be executed where the fixtures are made.  What
    vs_tweak, adjust_rgb, vs_rgb_normalize and rgb_denoise hand to those filters is the reference's Python, restated and pinned by tests/golden/tweak.npz.
    The `vs_tweak` refusals INSIDE the other entry points (HAVC_colorizer's sat / hue, HAVC_DeepRemaster / HAVC_restore_video render_vivid, ddtweak) stay exactly as they are: existing tests pin them, and routing them to the new code is a separate decision.
  * HAVC_TimeCube (vsdeoldify_amd/timecube.py has the details): the `timecube.Cube` plugin -> trilinear interpolation in the .cube file's table, float32, restated
    in tests/timecube_util.py, which csrc/lut3d.hip equals byte for byte -- the plugin is not in the reference tree.  The file names, the factors handed to
    vs_tweak and the merges are the reference's Python, restated and pinned by tests/golden/timecube.npz.  A LUT file that is not there is an ERROR here (the
    reference logs and goes on with the un-graded clip).  rgb_equalizer(method=4) / HAVC_bw_tune(bw_method=4) are not routed here yet and stay refused.
  * HAVC_clip_overlay (vsdeoldify_amd/overlay.py has the details): `std.Crop`, `std.AddBorders`, `std.Expr` and `std.MaskedMerge` -> the sequences of
    tests/overlay_util.py, which csrc/overlay.hip equals byte for byte; RGB24 only.
HAVC_clip_slice pads where the reference's std.CropAbs would leave the padded clip by one pixel (an odd width / height with overlap 0: VapourSynth
raises there); every other geometry CropAbs refuses -- an overlap >= the base tile, a negative overlap -- is refused with HAVCError.

The Placebo / VerySlow presets of HAVC_main (__init__.py:760-767, 862-870) on a clip, host or device:

    ox, oy, rf = tiled_preset_params(width, height, slices)                          # slices: 4 = Placebo, 2 = VerySlow
    clips = HAVC_clip_slice(clip, slices=slices, overlap_x=ox, overlap_y=oy)
    for i in range(slices): clips.tiles[i] = HAVC_colorizer(clips.tiles[i], deoldify_p=(0, rf, 1.0, 0.0), ddcolor_p=(1, rf, 1.0, 0.0, True), ...)
    out = HAVC_clip_reconstruct(clips, blend_weight=0, chroma_resize=True)

    out = HAVC_colorizer(clip, method=2, mweight=0.4, torch_dir=..., ...)          # clip: uint8 [n, 1080, 1920, 3]
    col = HAVCFrameColorizer(method=2, mweight=0.4, package_dir=...); out = col.colorize(frame)
"""
import dataclasses
import math
import os

import numpy as np

from . import _native as nat
from .precision import DEFAULT_PRECISION, resolve as resolve_precision
from . import imfilters as F
from . import mcomb
from .device import DeviceImage, is_device
from .render import get_context

DEF_CMC_p = [0.15, True, 20, 24]            # vsslib/constants.py:19-22
DEF_LMM_p = [0.15, 0.65, 1.0]
DEF_ALM_p = [0.8, 1.0, 0.15]
DEF_CRT_p = [0.8, 30, 2, False, 0, 0]
DEF_TWEAK_p = [0.0, 1.0, 2.5, True, 0.3, 0.6, 1.5, 0.5]     # vsslib/constants.py:23
DEF_THT_WHITE, DEF_THT_BLACK = 0.88, 0.12
DEF_STABLE_WEIGHT = DEF_ARTISTIC_WEIGHT = 0.5  # vsslib/constants.py:56-57


class HAVCError(ValueError):
    """what the reference raises as vs.Error / HAVC_LogMessage(EXCEPTION)"""


def _as_clip(x):
    """-> (4-D operand, was_single_frame)"""
    if is_device(x):
        return (x, False) if x.ndim == 4 else (x.reshaped((1,) + x.shape), True)
    a = np.ascontiguousarray(x, dtype=np.uint8)
    if a.ndim == 3:
        a, single = a[None], True
    else:
        single = False
    if a.ndim != 4 or a.shape[3] != 3:
        raise HAVCError("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    return a, single


class HAVCFrameColorizer:
    def __init__(self, method=2, mweight=0.4, deoldify_p=(0, 24, 1.0, 0.0), ddcolor_p=(1, 24, 1.0, 0.0, True), cmc_p=DEF_CMC_p,
                 lmm_p=DEF_LMM_p, alm_p=DEF_ALM_p, crt_p=DEF_CRT_p, cmb_sw=False, device_index=0, package_dir=None,
                 ddcolor_model_dir=None, state_dicts=None, ddcolor_state_dict=None, zhang_state_dict=None, max_batch=1,
                 ddcolor_kwargs=None, ddtweak=(False, False, False), ddtweak_p=(DEF_TWEAK_p, "none"), precision=None):
        """precision: "fast" / "precise" for EVERY model of the graph (DeOldify, DDColor, the Zhang colorizers): the reference runs them all in fp32
        (deoldify/filters.py:45-68, vsslib/vsmodels.py:353-363, colorization/__init__.py:76-95); None reads HAVC_PRECISION, then the package default "precise" (vsdeoldify_amd/precision.py)."""
        try:
            self.precision = resolve_precision(precision)        # explicit > HAVC_PRECISION > "precise" (vsdeoldify_amd/precision.py)
        except ValueError as e:
            raise HAVCError(f"HAVC: {e}") from None
        # ---- __init__.py:2452-2462: method <-> merge weight normalisation ----
        merge_weight = 0.0 if method == 0 else (1.0 if method == 1 else mweight)
        if merge_weight == 0.0:
            method = 0
        elif merge_weight == 1.0:
            method = 1
        if method not in range(0, 8):
            raise HAVCError("HAVC: only dd_method in (0,6) is supported")                        # mcomb.py:192
        self.method, self.merge_weight, self.cmb_sw = method, merge_weight, cmb_sw
        self._read_ddtweak(ddtweak, ddtweak_p)                   # refuses what only VapourSynth can do before anything touches the GPU
        self.deoldify_model, self.deoldify_rf, d_sat, d_hue = deoldify_p[:4]
        self.ddcolor_model, self.ddcolor_rf, c_sat, c_hue = ddcolor_p[:4]
        if device_index > 7:
            raise HAVCError("HAVC_colorizer: wrong device_index, choices are: GPU0...GPU7 (CPU=99 is not supported by this library)")
        if self.ddcolor_rf != 0 and self.ddcolor_rf not in range(10, 65):
            raise HAVCError("HAVC_colorizer: ddcolor render_factor must be between: 10-64")       # __init__.py:2482-2483
        if (d_sat, d_hue) != (1.0, 0.0) and method != 1 or (c_sat, c_hue) != (1.0, 0.0) and method != 0:
            raise NotImplementedError("sat / hue of deoldify_p / ddcolor_p go through vs_tweak (VapourSynth std.Expr + zimg): not in this harness")
        self.cmc_p, self.lmm_p, self.alm_p, self.crt_p = list(cmc_p), list(lmm_p), list(alm_p), list(crt_p)
        if method == 4 and self.lmm_p[2] < 1:
            raise NotImplementedError("luma_mask_sat < 1 uses vs_tweak (VapourSynth): not in this harness")
        self.device_index, self.ctx = device_index, get_context(device_index)
        self.max_batch = max_batch
        self._package_dir, self._dd_dir = package_dir, ddcolor_model_dir
        self._sds, self._dd_sd, self._zh_sd = state_dicts, ddcolor_state_dict, zhang_state_dict
        self._dd_kwargs = dict(ddcolor_kwargs or {})
        self._deoldify = self._ddcolor = self._zhang = None
        self._dd_size = None
        # Methods that run BOTH models on a device clip run them side by side: DDColor on a context (HIP stream) of its own, from a second
        # thread, while DeOldify runs on this one -- two independent chains of launches fill the chip better than one after the other
        # (HAVC_OVERLAP_MODELS=0: one after the other on one stream).  Same bytes either way.
        self.overlap_models = os.environ.get("HAVC_OVERLAP_MODELS", "1") != "0"
        self._pool = None

    def _read_ddtweak(self, flags, tweaks):
        """vs_sc_ddcolor's tweak handling WITHOUT scene detection (vsslib/vsmodels.py:304-344,365-374; scenechange = False because
        sc_threshold = sc_min_freq = 0, __init__.py:2496): what can be computed without VapourSynth is computed, the rest is refused.
          * hue_adjust (ddtweak_p[1], HAVC_colorizer's default "300:360|0.8,0.1"): adjust_hue_range on EVERY DDColor frame — applied;
          * tweaks_enabled with luma_constrained_tweak and neutral bright / cont (the DEF_TWEAK_p defaults): luma_adjusted_levels on every
            frame in front of DDColor, the source's luma put back behind it (vs_recover_clip_luma) — applied;
          * bright / cont / gamma through vs_tweak (std.Expr / std.Levels), rgb_denoise, vs_auto_levels (retinex): VapourSynth filters — refused."""
        flags = list(flags) if isinstance(flags, (list, tuple)) else [flags, False, False]
        self.dd_tweaks_enabled, denoise, retinex = (bool(f) for f in (flags + [False, False])[:3])
        if len(tweaks) == 2:
            t, hue_adjust = list(tweaks[0]), str(tweaks[1]).lower()
        else:
            t, hue_adjust = list(tweaks[:8]), (tweaks[8] if len(tweaks) > 8 else "none")
        self.dd_hue_adjust = hue_adjust
        self.dd_levels = None
        if denoise:
            raise NotImplementedError("ddtweak[1] (rgb_denoise) is a VapourSynth filter chain: not in this harness")
        if self.dd_tweaks_enabled:
            bright, cont, gamma, constrained, luma_min, gamma_luma_min, gamma_alpha, gamma_min = t[:8]
            if retinex:
                raise NotImplementedError("ddtweak[2] (vs_auto_levels / retinex) is a VapourSynth filter chain: not in this harness")
            if not constrained or bright != 0 or cont != 1:
                raise NotImplementedError("without scene detection vs_sc_tweak is vs_tweak (std.Expr / std.Levels): only the luma-constrained tweak "
                                          "with neutral bright / cont (the defaults) is computed here")
            self.dd_levels = (luma_min, gamma, gamma_luma_min, gamma_alpha, gamma_min)

    def _ddcolor_branch(self, sq, input_size, ctx=None):
        """vs_sc_ddcolor (vsmodels.py:290-375) on the squashed clip: [pre-tweak ->] DDColor / Zhang [-> hue adjust] [-> luma of the clip back].
        ctx: the context the branch's filters run on (the DDColor context when the two models run side by side)"""
        ctx = ctx or self.ctx
        src = sq
        if self.dd_levels is not None:                                # sc_constrained_tweak(scenechange=False): luma_adjusted_levels per frame
            frames = [F.luma_adjusted_levels_np(ctx, sq.frame(i) if is_device(sq) else sq[i], *self.dd_levels) for i in range(sq.shape[0])]
            if is_device(sq):
                src = DeviceImage(ctx, sq.shape)
                for i, f in enumerate(frames):
                    src.frame(i).copy_from(f)
            else:
                src = np.stack(frames)
        b = self._ddcolor_clip(src, input_size)
        if self.dd_hue_adjust not in ("none", ""):
            b = F.adjust_hue_range_np(ctx, b if is_device(b) else b.reshape((-1,) + b.shape[2:]), self.dd_hue_adjust)
            if not is_device(b):
                b = b.reshape(sq.shape)
        if self.dd_tweaks_enabled:
            b = F.chroma_post_process_np(ctx, b if is_device(b) else b.reshape((-1,) + b.shape[2:]),
                                         sq if is_device(sq) else sq.reshape((-1,) + sq.shape[2:]))
            if not is_device(b):
                b = b.reshape(sq.shape)
        return b

    # ---- model routing: vsslib/vsmodels.py:196-213 (deoldify), :290-350 (ddcolor / zhang) ----
    def _deoldify_render(self):
        if self._deoldify is None:
            from .render import ModelImageRender
            name, w = {0: ("video", 0), 1: ("stable", DEF_STABLE_WEIGHT), 2: ("artistic", DEF_ARTISTIC_WEIGHT)}.get(self.deoldify_model, ("video", 0))
            self._deoldify = ModelImageRender(self._package_dir, name, self.deoldify_rf, video_weight=w, device_index=self.device_index,
                                              state_dicts=self._sds, max_batch=self.max_batch, precision=self.precision)
        return self._deoldify

    def _ddcolor_model(self, input_size):
        if self._ddcolor is None or self._dd_size != input_size:
            from .ddcolor import DDColorRender
            kw = dict(self._dd_kwargs)
            if self._side_by_side():
                kw.setdefault("worker", ("havc-ddcolor", 0))
            kw.setdefault("precision", self.precision)
            self._ddcolor = DDColorRender(self.ddcolor_model, input_size, self.device_index, state_dict=self._dd_sd, model_dir=self._dd_dir, **kw)
            self._dd_size = input_size
        return self._ddcolor

    def _ddcolor_clip(self, sq, input_size):
        """sq: [n, fs, fs, 3] ndarray or DeviceImage -> same kind"""
        if self.ddcolor_model in (0, 1):
            return self._ddcolor_model(input_size).colorize_frames(sq, max_batch=self.max_batch)
        from .colorization import ModelColorization                                               # vsmodels.py:346-350
        if self._zhang is None:
            self._zhang = ModelColorization("siggraph17" if self.ddcolor_model == 2 else "eccv16", True, self.device_index, state_dict=self._zh_sd,
                                            precision=self.precision)
        return self._zhang.colorize_frames(sq)                                                    # host or device clip: havc_zhang_frames takes both

    def _side_by_side(self):
        return self.overlap_models and self.method not in (0, 1) and self.ddcolor_model in (0, 1)

    def _deoldify_clip(self, sq):
        """ModelImageRender over a clip.  Frames at the model's render size (the usual case: frame_size is derived from the larger
        render factor) run as device batches; any other size goes frame by frame through get_transformed_image, which squashes /
        un-squashes with Pillow BILINEAR on the host exactly where the reference does (deoldify/filters.py:37-41,70-73)."""
        from PIL import Image
        r = self._deoldify_render()
        S = self.deoldify_rf * 16
        if tuple(sq.shape[1:3]) == (S, S):
            return r.render_square_batch(sq)
        host = sq.numpy() if is_device(sq) else sq
        out = np.stack([np.asarray(r.get_transformed_image(Image.fromarray(f))) for f in host])
        return DeviceImage.from_numpy(self.ctx, out) if is_device(sq) else out

    def frame_size(self, width):
        """__init__.py:2490-2502."""
        dd_rf = self.ddcolor_rf or min(max(math.trunc(0.4 * width / 16), 16), 32)
        return dd_rf, min(max(dd_rf, self.deoldify_rf) * 16, width)

    def _spline64(self, img, w, h, luma_from=None):
        return spline64(self.ctx, img, w, h, luma_from)

    # ---- vsslib/mcomb.py:125-192 ----
    def _combine(self, a, b):
        return combine_models(a, b, self.method, self.merge_weight, self.cmc_p, self.lmm_p, self.alm_p, self.crt_p, self.cmb_sw, self.device_index)

    def colorize_clip(self, clip):
        """HAVC_colorizer's graph on a clip: Spline64 squash -> deoldify / ddcolor -> combine -> Spline64 back + luma of the source
        (_clip_chroma_resize, __init__.py:3545-3554).  ndarray in -> ndarray out; DeviceImage in -> DeviceImage out (nothing leaves
        HBM; frames go through the models in batches of max_batch)."""
        clip, single = _as_clip(clip)
        n, h, w, _ = clip.shape
        dd_rf, fs = self.frame_size(w)
        host_in = not is_device(clip)
        dclip = DeviceImage.from_numpy(self.ctx, clip) if host_in else clip
        sq = dclip if (w, h) == (fs, fs) else self._spline64(dclip, fs, fs)
        a = b = None
        dd_size = math.trunc(dd_rf / 2) * 32                                                      # vsmodels.py:302
        if self._side_by_side() and is_device(sq):
            # The two models side by side on two contexts, DDColor driven from a second thread -- from the first clip on: building the models,
            # their nets and the tile autotuning from two host threads at once is serialised INSIDE the library (the set-up mutex of
            # csrc/rt_context.cpp; the reference's glue builds models from whichever worker thread asks first, vsslib/vsmodels.py:196-233).
            import concurrent.futures
            if self._pool is None:
                self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
            self.ctx.synchronize()                                                                # the squashed clip is complete: the other context may read it

            def branch():
                bctx = self._ddcolor_model(dd_size).rt.ctx
                try:
                    return self._ddcolor_branch(sq, dd_size, bctx)
                finally:
                    bctx.synchronize()                                                            # (only enqueued: this context must not run ahead of it)
            fut = self._pool.submit(branch)
            err = None
            try:
                a = self._deoldify_clip(sq)
            except BaseException as e:                                                            # noqa: BLE001 -- re-raised below, after the branch has drained
                err = e
            try:
                b = fut.result()          # ALWAYS waited for: the branch's stream reads `sq`, whose buffer returns to this context's pool when we leave
            except BaseException as e:                                                            # noqa: BLE001
                err = err or e
            if err is not None:
                raise err
        else:
            if self.method != 1:
                a = self._deoldify_clip(sq)
            if self.method != 0:
                b = self._ddcolor_branch(sq, dd_size, None)
        col = self._combine(a, b)
        out = self._spline64(col, w, h, luma_from=dclip)
        if host_in:
            out = out.numpy()
        return (out[0] if host_in else out.reshaped(out.shape[1:])) if single else out

    def colorize(self, frame):
        """one uint8 [h, w, 3] frame (or a clip) through the graph"""
        return self.colorize_clip(frame)

    __call__ = colorize_clip


def spline64(ctx, img, w, h, luma_from=None):
    """the harness stand-in of `resize.Spline64` (+ vs_recover_clip_luma when luma_from is given) on frames or clips,
    host or device operands"""
    return _resize(ctx, img, w, h, luma_from, None)


def spline36(ctx, img, w, h, luma_from=None):
    """the harness stand-in of `resize.Spline36`: the same passes with the Spline36 kernel (havc_resize_n)"""
    return _resize(ctx, img, w, h, luma_from, nat.RESIZE_SPLINE36)


def _resize(ctx, img, w, h, luma_from, filter_id):
    dev = is_device(img) or is_device(luma_from)
    if dev:
        img = img if is_device(img) else DeviceImage.from_numpy(ctx, img)
        if luma_from is not None and not is_device(luma_from):
            luma_from = DeviceImage.from_numpy(ctx, luma_from)
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        luma_from = None if luma_from is None else np.ascontiguousarray(luma_from, dtype=np.uint8)
    n = img.shape[0] if img.ndim == 4 else 1
    sh, sw = img.shape[-3], img.shape[-2]
    shape = ((n, h, w, 3) if img.ndim == 4 else (h, w, 3))
    if luma_from is not None and tuple(luma_from.shape) != shape:
        raise ValueError("luma_from must have the output shape")
    out = DeviceImage(ctx, shape) if dev else np.empty(shape, np.uint8)
    from .device import operand_ptr
    args = (ctx.h, operand_ptr(img), sw, sh, operand_ptr(out), w, h, operand_ptr(luma_from) if luma_from is not None else None, n)
    nat.check(ctx.lib.havc_spline64_resize_n(*args) if filter_id is None else ctx.lib.havc_resize_n(*args, filter_id), ctx.h)
    return out


def _per_frame(fn, *clips):
    """apply a frame-level function (frame statistics / neighbourhoods inside) to every frame of 4-D operands"""
    first = clips[0]
    n = first.shape[0]
    if is_device(first):
        out = first.empty_like()
        for i in range(n):
            out.frame(i).copy_from(fn(*[c.frame(i) for c in clips]))
        return out
    return np.stack([np.asarray(fn(*[c[i] for c in clips])) for i in range(n)])


def combine_models(a, b, method, w, cmc_p=DEF_CMC_p, lmm_p=DEF_LMM_p, alm_p=DEF_ALM_p, crt_p=DEF_CRT_p, invert_clips=False, device_index=0):
    """vs_sc_combine_models (vsslib/mcomb.py:125-192) on clips [n, h, w, 3] (ndarray or DeviceImage); sat / hue tweaks refused
    by the callers.  Purely per-pixel methods run on the whole stack in one launch, methods with frame-level decisions (mean
    luma, Laplacian) frame by frame."""
    if invert_clips:
        a, b = b, a
    if a is None or b is None:
        return a if b is None else b
    di = device_index
    big = len(cmc_p) > 1
    red_fix = cmc_p[1] if big else True
    rows = (lambda x: x.as_rows()) if is_device(a) else (lambda x: x.reshape((-1,) + x.shape[2:]))
    unrows = (lambda x: x.reshaped(a.shape)) if is_device(a) else (lambda x: x.reshape(a.shape))
    if method == 2:
        return unrows(mcomb.simple_merge(rows(a), rows(b), w, di))
    if method == 3:
        ccm = _per_frame(lambda x, y: mcomb.constrained_chroma_merge(x, y, w, cmc_p[0], red_fix, di), a, b)
        mm = mcomb.simple_merge(rows(a), rows(b), min(w, 0.6), di)
        return unrows(mcomb.simple_merge(rows(ccm), mm, 0.3, di))
    if method == 4:
        return unrows(mcomb.luma_masked_merge(rows(a), rows(b), None, lmm_p[0], lmm_p[1], w, di))
    if method == 5:
        return _per_frame(lambda x, y: mcomb.adaptive_luma_merge(x, y, alm_p[0], alm_p[1], w, alm_p[2], di), a, b)
    if method == 6:
        if crt_p[3]:                                                         # chroma_resize: the whole of ChromaRetentionMerge on the clip (Spline64 stand-in)
            return mcomb.chroma_retention_merge_clip(a, b, crt_p[0], crt_p[1], w, crt_p[2], crt_p[4], True, False, False, crt_p[5], 0, di)
        restored = _per_frame(lambda x, y: mcomb.chroma_retention_frame(x, y, crt_p[0], crt_p[1], crt_p[4], crt_p[2], False, crt_p[5], di), a, b)
        return unrows(mcomb.simple_merge(rows(a), rows(restored), w, di))   # vs_simple_merge = std.Merge in the reference (VapourSynth core)
    if method == 7:
        return _per_frame(lambda x, y: mcomb.chroma_bound_adaptive_merge(x, y, red_fix, cmc_p[2] if big else 20, cmc_p[3] if big else 24, w, di), a, b)
    raise HAVCError("HAVC: only dd_method in (0,6) is supported")


# ======================================================================================================================
# function-shaped API (argument lists of the reference)
# ======================================================================================================================
_colorizers = {}


def _refuse_vs_only(ddtweak, sc_threshold, sc_min_freq):
    if sc_threshold and sc_threshold > 0 or sc_min_freq and sc_min_freq > 0:
        raise NotImplementedError("scene detection (sc_threshold / sc_min_freq) is VapourSynth glue (SCDetect): not in this harness")


def HAVC_colorizer(clip, method=2, mweight=0.4, deoldify_p=(0, 24, 1.0, 0.0), ddcolor_p=(1, 24, 1.0, 0.0, True), ddtweak=(False, False, False),
                   ddtweak_p=(DEF_TWEAK_p, "300:360|0.8,0.1"), cmc_p=DEF_CMC_p, lmm_p=DEF_LMM_p, alm_p=DEF_ALM_p, crt_p=DEF_CRT_p, cmb_sw=False,
                   sc_threshold=0.0, sc_tht_offset=1, sc_min_freq=0, sc_tht_ssim=0.0, sc_normalize=False, sc_min_int=1, sc_tht_white=DEF_THT_WHITE,
                   sc_tht_black=DEF_THT_BLACK, device_index=0, torch_dir=None, debug_level=0, **harness):
    """vsdeoldify/__init__.py:2290-2298.  `harness` = keyword-only extras of this library: state_dicts / ddcolor_state_dict /
    zhang_state_dict (seeded weights instead of files under torch_dir), ddcolor_model_dir, max_batch, ddcolor_kwargs, precision ("fast" / "precise")."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_colorizer: this is not a clip")                                     # __init__.py:2437-2438
    _refuse_vs_only(ddtweak, sc_threshold, sc_min_freq)
    cmc = list(cmc_p) if isinstance(cmc_p, (list, tuple)) else [cmc_p]
    flags = tuple(ddtweak) if isinstance(ddtweak, (list, tuple)) else (ddtweak, False, False)
    key = (method, mweight, tuple(deoldify_p), tuple(ddcolor_p), tuple(cmc), tuple(lmm_p), tuple(alm_p), tuple(crt_p), cmb_sw, device_index,
           torch_dir, id(harness.get("state_dicts")), id(harness.get("ddcolor_state_dict")), harness.get("max_batch", 1), flags, repr(ddtweak_p),
           harness.get("precision") or os.environ.get("HAVC_PRECISION") or DEFAULT_PRECISION)
    col = _colorizers.get(key)
    if col is None:
        col = HAVCFrameColorizer(method, mweight, deoldify_p, ddcolor_p, cmc, lmm_p, alm_p, crt_p, cmb_sw, device_index, package_dir=torch_dir,
                                 ddtweak=flags, ddtweak_p=ddtweak_p, **harness)
        _colorizers.clear()                     # one live graph at a time: the nets hold GBs of activations
        _colorizers[key] = col
    return col.colorize_clip(clip)


def HAVC_ddeoldify(clip, method=2, mweight=0.4, deoldify_p=(0, 24, 1.0, 0.0), ddcolor_p=(1, 24, 1.0, 0.0, True), ddtweak=False,
                   ddtweak_p=(DEF_TWEAK_p, "300:360|0.8,0.1"), cmc_tresh=0.2, lmm_p=(0.2, 0.8, 1.0), alm_p=(0.8, 1.0, 0.15), cmb_sw=False,
                   sc_threshold=0.0, sc_tht_offset=1, sc_min_freq=0, sc_tht_ssim=0.0, sc_normalize=False, sc_min_int=1, sc_tht_white=DEF_THT_WHITE,
                   sc_tht_black=DEF_THT_BLACK, device_index=0, torch_dir=None, sc_debug=False, **harness):
    """deprecated wrapper, vsdeoldify/__init__.py:3612-3628: the same call with cmc_p = [cmc_tresh] and DEF_CRT_p"""
    import warnings
    warnings.warn("Warning: HAVC_ddeoldify is deprecated and may be removed in the future, please use 'HAVC_colorizer' instead.", DeprecationWarning)
    return HAVC_colorizer(clip, method, mweight, deoldify_p, ddcolor_p, [ddtweak, False, False], ddtweak_p, [cmc_tresh], lmm_p, alm_p, DEF_CRT_p, cmb_sw,
                          sc_threshold, sc_tht_offset, sc_min_freq, sc_tht_ssim, sc_normalize, sc_min_int, sc_tht_white, sc_tht_black, device_index,
                          torch_dir, 1 if sc_debug else 0, **harness)


def ddeoldify(clip, method=2, mweight=0.4, deoldify_p=(0, 24, 1.0, 0.0), ddcolor_p=(1, 24, 1.0, 0.0, True), dotweak=False,
              dotweak_p=(0.0, 1.0, 1.0, False, 0.2, 0.5, 1.5, 0.5), ddtweak=False, ddtweak_p=(DEF_TWEAK_p, "300:360|0.8,0.1"), degrain_strength=0,
              cmc_tresh=0.2, lmm_p=(0.2, 0.8, 1.0), alm_p=(0.8, 1.0, 0.15), cmb_sw=False, device_index=0, torch_dir=None, **harness):
    """deprecated wrapper, vsdeoldify/__init__.py:3642-3653 (dotweak / degrain_strength are accepted and ignored, as there)"""
    import warnings
    warnings.warn("Warning: ddeoldify is deprecated and may be removed in the future, please use 'HAVC_colorizer' instead.", DeprecationWarning)
    return HAVC_colorizer(clip, method, mweight, deoldify_p, ddcolor_p, [ddtweak, False, False], ddtweak_p, [cmc_tresh], lmm_p, alm_p, DEF_CRT_p, cmb_sw,
                          sc_threshold=0, sc_min_freq=0, device_index=device_index, torch_dir=torch_dir, **harness)


def _clip_chroma_resize(clip_hires, clip_lowres, device_index=0):
    """__init__.py:3545-3554: Spline64 to the hi-res size, then vs_recover_clip_luma (luma of clip_hires, chroma of the resized)"""
    hi, _ = _as_clip(clip_hires)
    lo, _ = _as_clip(clip_lowres)
    return spline64(get_context(device_index), lo, hi.shape[2], hi.shape[1], luma_from=hi)


def HAVC_merge(clipa=None, clipb=None, clip_luma=None, weight=0.5, method=2, cmc_p=DEF_CMC_p, lmm_p=DEF_LMM_p, alm_p=DEF_ALM_p, crt_p=DEF_CRT_p,
               device_index=0):
    """vsdeoldify/__init__.py:2536-2675: the HAVC merge methods on two already coloured clips (+ optional luma source)."""
    for name, c in (("clipa", clipa), ("clipb", clipb), ("clip_luma", clip_luma)):
        if c is not None and not (is_device(c) or isinstance(c, np.ndarray)):
            raise HAVCError(f"HAVC_merge: this is not a clip: {name}")                           # __init__.py:2631-2638
    single = (clipa if clipa is not None else clipb).ndim == 3

    def done(x):
        if single and x.ndim == 4:
            return x.reshaped(x.shape[1:]) if is_device(x) else x[0]
        return x
    if method == 0 or weight == 0:                                                                # __init__.py:2640-2645
        return done(_clip_chroma_resize(clip_luma, clipa, device_index)) if clip_luma is not None else clipa
    if method == 1 or weight == 1:                                                                # __init__.py:2647-2652
        return done(_clip_chroma_resize(clip_luma, clipb, device_index)) if clip_luma is not None else clipb
    a, _ = _as_clip(clipa)
    b, _ = _as_clip(clipb)
    if is_device(a) != is_device(b):
        ctx = get_context(device_index)
        a = a if is_device(a) else DeviceImage.from_numpy(ctx, a)
        b = b if is_device(b) else DeviceImage.from_numpy(ctx, b)
    if method == 2:                                                                               # __init__.py:2659-2661
        return done(combine_models(a, b, 2, weight, device_index=device_index))
    if clip_luma is not None:                                                                     # __init__.py:2663-2667
        luma, _ = _as_clip(clip_luma)
        rf = min(max(math.trunc(0.4 * luma.shape[2] / 16), 16), 32)
        fs = min(rf * 16, luma.shape[2])
        ctx = get_context(device_index)
        a, b = spline64(ctx, a, fs, fs), spline64(ctx, b, fs, fs)
    cmc = list(cmc_p) if isinstance(cmc_p, (list, tuple)) else [cmc_p]
    merged = combine_models(a, b, method, weight, cmc, lmm_p, alm_p, crt_p, False, device_index)  # vs_combine_models(sat=[1,1], hue=[0,0])
    if clip_luma is not None:                                                                     # __init__.py:2673-2676
        merged = _clip_chroma_resize(clip_luma, merged, device_index)
    return done(merged)


# ---- HAVC_recover_clip_color (vsdeoldify/__init__.py:2956-2992) ---------------------------------------------------------------------------------
def HAVC_recover_clip_color(clip=None, clip_color=None, sat=0.8, tht=30, strength=1.0, alpha=2.0, mask_weight=1.0, chroma_resize=True, return_mask=False,
                            binary_mask=False, algo=0, *, device_index=0):
    """vsdeoldify/__init__.py:2956-2992: restore the colours of the gray pixels of `clip` with those of `clip_color` ("useful to repair the clips colored with
    DeepRemaster") = ChromaRetentionMerge(clip, clip_color, sat, tht, clipb_weight=strength, alpha, mask_weight, scenechange=False, chroma_resize, return_mask,
    binary_mask, algo) -> mcomb.chroma_retention_merge_clip: one havc_recover_color_clip call (two launches over the whole clip) between the Spline64 round
    trip of chroma_resize and the closing merge.  ndarray in -> ndarray out; DeviceImage in -> DeviceImage out (nothing leaves HBM, the call only enqueues);
    one of each: the ndarray is uploaded.  A frame [h, w, 3] in -> a frame out.  Frame 0 of the operand is clip frame 0 (the binary selector's `n < 15`)."""
    for c in (clip, clip_color):                                                                  # __init__.py:2983-2984 (the text names HAVC_merge there)
        if c is None or not (is_device(c) or isinstance(c, np.ndarray)):
            raise HAVCError("HAVC_merge: this is not a clip: clip_color")
    for c in (clip, clip_color):
        if c.ndim not in (3, 4) or c.shape[-1] != 3 or (not is_device(c) and c.dtype != np.uint8):
            raise HAVCError("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    if tuple(clip.shape) != tuple(clip_color.shape):
        raise HAVCError(f"HAVC_recover_clip_color: clip {tuple(clip.shape)} and clip_color {tuple(clip_color.shape)} differ in size")
    if algo not in (0, 1, 2):
        raise HAVCError(f"HAVC_recover_clip_color: algo = {algo}: only 0, 1, 2 are supported")
    a, single = _as_clip(clip)
    b, _ = _as_clip(clip_color)
    out = mcomb.chroma_retention_merge_clip(a, b, sat, tht, strength, alpha, mask_weight, chroma_resize, return_mask, binary_mask, algo, 0, device_index)
    if is_device(out):
        return out.reshaped(out.shape[1:]) if single else out
    return out[0] if single else out


# ---- HAVC_stabilizer (vsdeoldify/__init__.py:2748-2873) ----------------------------------------------------------------------------------------
_COLORMAPS = ['none', 'blue->brown', 'blue->red', 'blue->green', 'green->brown', 'green->red', 'green->blue', 'redrose->brown', 'redrose->blue',
              'red->brown', 'red->blue', 'yellow->rose']                                          # havc_utils.py:564-565
_COLORMAP_HUES = ["none", "180:280|+140", "180:280|+100", "180:280|+220", "80:180|+260", "80:180|+220", "80:180|+140", "300:360,0:20|+40",
                  "300:360,0:20|+260", "320:360|+50", "300:360|+260", "30:90|+300"]               # havc_utils.py:566-567


def _get_colormap(colormap):
    """havc_utils._get_colormap(ColorMap) with its default ColorTune = "light" (havc_utils.py:552-581): a known name -> its "chroma adjustment" with
    weight 0.90; a string parse_hue_adjust accepts is handed on; anything else is an error"""
    colormap = colormap.lower()
    if colormap in _COLORMAPS:
        return _COLORMAP_HUES[_COLORMAPS.index(colormap)] + "," + "0.90"
    if F.parse_hue_adjust(colormap) is None:
        raise HAVCError("HAVC_main: ColorMap choice is invalid for '" + colormap + "'")           # havc_utils.py:575
    return colormap


def _stabilizer_frame_size(render_factor, width):
    """__init__.py:2795-2803 -> (render_factor, frame_size)"""
    if render_factor != 0 and render_factor not in range(16, 65):
        raise HAVCError("HAVC_stabilizer: render_factor must be between: 16-64")                  # __init__.py:2795-2796
    if render_factor == 0:
        render_factor = min(max(math.trunc(0.4 * width / 16), 16), 32)                            # __init__.py:2798-2799
    return render_factor, min(render_factor * 16, width)                                          # __init__.py:2803


def HAVC_stabilizer(clip, dark=False, dark_p=(0.2, 0.8), smooth=False, smooth_p=(0.3, 0.7, 0.9, 0.0, "none"), stab=False,
                    stab_p=(5, 'A', 1, 15, 0.2, 0.8), colormap="none", render_factor=24, device_index=0):
    """vsdeoldify/__init__.py:2748-2751: the colour filters every HAVC_main preset ends in, at reduced resolution -- Spline64 squash to
    frame_size x frame_size (the library's Spline64, the stand-in of zimg's everywhere in this file), dark -> smooth -> colormap in ONE launch
    (stabilizer.stabilize_np), Spline64 back + the luma of the source (_clip_chroma_resize).  ndarray in -> ndarray out; DeviceImage in -> DeviceImage out
    (nothing leaves HBM, the call only enqueues).  stab=True (a clip only) adds vs_chroma_stabilizer_ex and vs_reduce_flicker behind the three
    (chroma_stab.stab_stage_np: havc_chroma_stab_clip; the stand-ins of zimg, std.AverageFrames and ReduceFlicker are defined by tests/stab_util.py).  Arrays
    carry no frame props, and this function keeps the reference's argument list: the clip is taken to have no scene changes; HAVC_stabilizer_scenes below
    is the same call with the SceneInfo of the clip.  Frame 0 of the operand is clip frame 0 (vs_sc_recover_clip_color's `n < 15`)."""
    return _stabilizer(clip, dark, dark_p, smooth, smooth_p, stab, stab_p, colormap, render_factor, device_index, None)


def HAVC_stabilizer_scenes(clip, scenes, dark=False, dark_p=(0.2, 0.8), smooth=False, smooth_p=(0.3, 0.7, 0.9, 0.0, "none"), stab=False,
                           stab_p=(5, 'A', 1, 15, 0.2, 0.8), colormap="none", render_factor=24, device_index=0):
    """HAVC_stabilizer on a clip whose scene changes are known: `scenes` is the SceneInfo of the clip (HAVC_SceneDetect's result for it, as in
    HAVC_export_reference_frames), what the reference's std.AverageFrames(scenechange=True) reads off every frame as _SceneChangePrev / _SceneChangeNext
    (stab=True with tht = stab_p[3] = 0, vs_clip_color_stabilizer; no other stage looks at them).  None = no scene changes."""
    return _stabilizer(clip, dark, dark_p, smooth, smooth_p, stab, stab_p, colormap, render_factor, device_index, scenes)


def _stabilizer(clip, dark, dark_p, smooth, smooth_p, stab, stab_p, colormap, render_factor, device_index, scenes):
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_stabilizer: this is not a clip")
    if stab and clip.ndim == 3:                                                                   # __init__.py:2862-2866
        raise NotImplementedError("HAVC_stabilizer(stab=True): vs_chroma_stabilizer_ex averages every frame with up to 14 neighbours and vs_reduce_flicker "
                                  "reads two frames on either side: a lone image [h, w, 3] has none -- pass a clip [n, h, w, 3]")
    clip, single = _as_clip(clip)
    n, h, w, _ = clip.shape
    _, fs = _stabilizer_frame_size(render_factor, w)
    if stab:                                                                                      # __init__.py:2834-2846
        from . import chroma_stab
        if len(stab_p) < 6:
            raise HAVCError("HAVC_stabilizer: stab_p needs (nframes, mode, sat, tht, weight, tht_scen[, hue adjust])")
        chroma_stab.weight_list(stab_p[0], stab_p[1])                                             # "HybridAVC: unknown average method: ..."
        if fs % 2:
            raise HAVCError(f"HAVC_stabilizer(stab=True): frame_size = {fs} is odd: the YUV420 round trip of vs_chroma_stabilizer_ex needs an even width "
                            f"and height (VapourSynth refuses it too)")
        if scenes is not None and len(scenes.scene_change_prev) != n:
            raise HAVCError("HAVC_stabilizer: scenes= must be the SceneInfo of this clip (AverageFrames reads _SceneChangePrev / _SceneChangeNext off "
                            "every frame)")
    dark_args = smooth_args = None
    if dark:                                                                                      # __init__.py:2806-2813, 2850-2852
        dark_args = (dark_p[0], dark_p[1], (dark_p[2] if len(dark_p) > 2 else "none").lower())
    if smooth:                                                                                    # __init__.py:2815-2824, 2854-2857
        smooth_args = (smooth_p[0], smooth_p[1], smooth_p[2], -smooth_p[3], (smooth_p[4] if len(smooth_p) > 4 else "none").lower())
    colormap = colormap.lower()                                                                   # __init__.py:2827-2832
    colormap_adjust = _get_colormap(colormap) if colormap not in ("none", "") else None
    if colormap_adjust is not None:
        # _get_colormap hands on ANY string without a "|" ("purple->green"); the reference then dies in the first frame's selector, inside
        # _parse_hue_range (restcolor.py:436-470).  Same refusal, raised here, before anything is enqueued.
        try:
            F.parse_hue_ranges(F.parse_hue_adjust(colormap_adjust)[0])
        except ValueError:
            raise HAVCError("HAVC_main: ColorMap choice is invalid for '" + colormap + "'") from None
    from .stabilizer import stabilize_np
    ctx = get_context(device_index)
    sq = spline64(ctx, clip, fs, fs)                                                              # __init__.py:2804
    col = stabilize_np(ctx, sq, dark_args, smooth_args, colormap_adjust)
    if stab:                                                                                      # __init__.py:2862-2866
        col = chroma_stab.stab_stage_np(ctx, col, stab_p, scenes=scenes)
    out = _clip_chroma_resize(clip, col, device_index)                                            # __init__.py:2868-2869: even when every filter is off
    if single:
        return out.reshaped(out.shape[1:]) if is_device(out) else out[0]
    return out


# ---- HAVC_clip_slice / HAVC_clip_reconstruct (vsdeoldify/__init__.py:2886-2945, vsslib/vstiles4.py) ----------------------------------------------------
@dataclasses.dataclass
class ClipTiles:
    """vstiles4.py:28-44.  `tiles` is a plain list: the caller replaces tiles[i] by the colorized tile (__init__.py:865)."""
    clip_orig: object              # original clip (ndarray, DeviceImage or None)
    tiles: list                    # [tl, tr, bl, br] or [tl, tr] -- each (base_tile_h + overlap_y) x (base_tile_w + overlap_x)
    base_tile_w: int               # base tile size (without the overlap)
    base_tile_h: int
    overlap_x: int                 # actual overlap in pixels
    overlap_y: int


def tiled_preset_params(width, height, slices):
    """(overlap_x, overlap_y, render_factor) of the Placebo (slices = 4) / VerySlow (slices = 2) presets, __init__.py:761-764: 20 % of half the clip,
    between 64 and 192 / 108 pixels, even; the render factor covers a tile's width.  HAVC_clip_slice ignores overlap_y for 2 tiles, as there."""
    overlap_x = (round(max(min((0.5 * width) * 0.2, 192), 64), 0) // 2) * 2
    overlap_y = (round(max(min((0.5 * height) * 0.2, 108), 64), 0) // 2) * 2
    render_factor = min(max(math.trunc((0.5 * width + overlap_x) / 16), 22), 32)
    return int(overlap_x), int(overlap_y), int(render_factor)


def _tile_geometry(w, h, slices, overlap_x, overlap_y):
    """vstiles4.py:72-83 / :132-141 -> (n_tiles, base_tile_w, base_tile_h, overlap_x, overlap_y); what std.CropAbs would refuse is refused here"""
    base_w = (w + 1) // 2
    overlap_x = int((overlap_x // 2) * 2)
    if slices == 4:
        n_tiles, base_h, overlap_y = 4, (h + 1) // 2, int((overlap_y // 2) * 2)
    else:                                                                                        # the reference's `else`: any other value = 2 tiles
        n_tiles, base_h, overlap_y = 2, h, 0
    if overlap_x < 0 or overlap_x >= base_w:
        raise HAVCError(f"HAVC_clip_slice: overlap_x = {overlap_x} must be >= 0 and smaller than the base tile width {base_w}")
    if overlap_y < 0 or (n_tiles == 4 and overlap_y >= base_h):
        raise HAVCError(f"HAVC_clip_slice: overlap_y = {overlap_y} must be >= 0 and smaller than the base tile height {base_h}")
    return n_tiles, base_w, base_h, overlap_x, overlap_y


def _tile_ctx(operands):
    for x in operands:
        if is_device(x):
            return x.ctx, True
    return get_context(0), False


def _tile_ptrs(tiles):
    import ctypes as C
    from .device import operand_ptr
    return (C.c_void_p * 4)(*[operand_ptr(t) for t in tiles])


def HAVC_clip_slice(clip, slices=2, overlap_x=32, overlap_y=32):
    """vsdeoldify/__init__.py:2886-2911: the clip cut into 4 (slices == 4: a 2 x 2 grid) or 2 (anything else: side by side) overlapping tiles; the clip is
    padded with black on the right / bottom by the overlaps (rounded down to even) first.  One launch writes every tile (havc_tile_slice).  ndarray in ->
    ndarray tiles; DeviceImage in -> DeviceImage tiles (nothing leaves HBM, the call only enqueues)."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_clip_slice: this is not a clip")
    orig = clip
    clip, single = _as_clip(clip)
    n, h, w, _ = clip.shape
    n_tiles, base_w, base_h, ox, oy = _tile_geometry(w, h, slices, overlap_x, overlap_y)
    ctx, dev = _tile_ctx([clip])
    shape = (n, base_h + oy, base_w + ox, 3)
    tiles = [DeviceImage(ctx, shape) if dev else np.empty(shape, np.uint8) for _ in range(n_tiles)]
    geom = nat.TileGeom(w, h, n, n_tiles, base_w, base_h, ox, oy, 0, 0)
    from .device import operand_ptr
    import ctypes as C
    nat.check(ctx.lib.havc_tile_slice(ctx.h, operand_ptr(clip), _tile_ptrs(tiles), C.byref(geom)), ctx.h)
    if single:
        tiles = [t.reshaped(t.shape[1:]) if dev else t[0] for t in tiles]
    return ClipTiles(clip_orig=orig, tiles=tiles, base_tile_w=base_w, base_tile_h=base_h, overlap_x=ox, overlap_y=oy)


def HAVC_clip_reconstruct(clip_tiles, blend_weight=0.5, chroma_resize=False):
    """vsdeoldify/__init__.py:2922-2945: the tiles blended back into one clip of clip_orig's size (vstiles4.py:161-348) -- rows (tl, tr) and (bl, br), then the
    two results as columns, each blend rounded to uint8; blend_weight 0 (mask value int(round(blend_weight * 255)) == 0) = a linear ramp over the overlap,
    otherwise that constant weight for the right / bottom tile; chroma_resize = the luma of clip_orig under the blend's chroma.  One launch
    (havc_tile_reconstruct).  Host and device operands may be mixed: any DeviceImage -> a DeviceImage comes back and the call only enqueues."""
    tiles = list(clip_tiles.tiles)
    if len(tiles) not in (2, 4):
        raise HAVCError(f"HAVC_clip_reconstruct: 2 or 4 tiles expected, got {len(tiles)}")
    for t in tiles:
        if t is None or not (is_device(t) or isinstance(t, np.ndarray)):
            raise HAVCError("HAVC_clip_reconstruct: this is not a clip: tiles")
    orig = clip_tiles.clip_orig
    if orig is None and chroma_resize:
        raise HAVCError("HAVC_clip_reconstruct: chroma_resize=True needs clip_orig (the luma source)")
    if orig is not None and not (is_device(orig) or isinstance(orig, np.ndarray)):
        raise HAVCError("HAVC_clip_reconstruct: this is not a clip: clip_orig")
    mask_val = int(round(blend_weight * 255))                                                     # vstiles4.py:284
    if not 0 <= mask_val <= 255:
        raise HAVCError("HAVC_clip_reconstruct: blend_weight must be between 0 and 1")
    base_w, base_h, ox, oy = (int(v) for v in (clip_tiles.base_tile_w, clip_tiles.base_tile_h, clip_tiles.overlap_x, clip_tiles.overlap_y))
    ox, oy = max(ox, 0), max(oy, 0)                                                               # overlap <= 0: plain stacking (vstiles4.py:316-317, 337-338)
    single = tiles[0].ndim == 3
    tiles = [_as_clip(t)[0] for t in tiles]
    n = tiles[0].shape[0]
    if len(tiles) == 2:
        oy = 0
    full_w, full_h = 2 * base_w, (2 * base_h if len(tiles) == 4 else base_h)
    if base_w <= 0 or base_h <= 0 or ox >= base_w or (len(tiles) == 4 and oy >= base_h):
        raise HAVCError("HAVC_clip_reconstruct: an overlap must be smaller than the base tile")
    for t in tiles:
        if tuple(t.shape) != (n, base_h + oy, base_w + ox, 3):
            raise HAVCError(f"HAVC_clip_reconstruct: a tile of shape {tuple(t.shape)} does not match base tile + overlap = {(n, base_h + oy, base_w + ox, 3)}")
    if orig is not None:
        orig, _ = _as_clip(orig)
        if orig.shape[0] != n or orig.shape[2] > full_w or orig.shape[1] > full_h or (len(tiles) == 2 and orig.shape[1] != full_h):
            raise HAVCError(f"HAVC_clip_reconstruct: clip_orig of shape {tuple(orig.shape)} is not covered by the tiles ({n} frames of {full_h} x {full_w})")
        h, w = orig.shape[1:3]
    else:
        h, w = full_h, full_w
    ctx, dev = _tile_ctx(tiles + [orig])
    out = DeviceImage(ctx, (n, h, w, 3)) if dev else np.empty((n, h, w, 3), np.uint8)
    geom = nat.TileGeom(w, h, n, len(tiles), base_w, base_h, ox, oy, mask_val, 1 if chroma_resize else 0)
    from .device import operand_ptr
    import ctypes as C
    nat.check(ctx.lib.havc_tile_reconstruct(ctx.h, _tile_ptrs(tiles), operand_ptr(orig) if chroma_resize else None, operand_ptr(out), C.byref(geom)), ctx.h)
    if single:
        return out.reshaped(out.shape[1:]) if dev else out[0]
    return out


# ---- HAVC_SceneDetect (vsdeoldify/__init__.py:3191-3225 -> vsslib/vsscdect.py) --------------------------------------------------------------------------
def HAVC_SceneDetect(clip, sc_threshold=0.10, sc_tht_offset=1, sc_tht_ssim=0.0, sc_min_int=1, sc_min_freq=0, sc_normalize=False, sc_tht_white=0.70,
                     sc_tht_black=0.10, sc_debug=False, *, device_index=0, luma_range="limited"):
    """vsdeoldify/__init__.py:3191-3225: the scene-change frames of a clip.  The reference sets frame props; arrays carry none, so the props come back as a
    `scdetect.SceneInfo` (scene_change_prev / scene_change_next / sc_luma / sc_ratio per frame + sc_threshold / sc_frequency).  The per-frame statistics
    are ONE launch over the clip (havc_scene_stats; two with sc_normalize); a DeviceImage stays in HBM and only the per-frame records come back.  The
    decision is scdetect.scene_flags, on the host.  sc_debug is accepted and ignored.  luma_range ("limited" / "full") picks the gray conversion's
    coefficients (module docstring).  The SSIM post-filter is refused HERE before anything is enqueued (tests/test_scdetect_host.py pins that); it is built as
    scdetect.scene_detect_filtered and runs in HAVC_extract_reference_frames."""
    from . import scdetect
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_SceneDetect: this is not a clip")
    if luma_range not in ("limited", "full"):
        raise HAVCError("HAVC_SceneDetect: luma_range must be 'limited' or 'full'")
    branch = scdetect.detect_branch(sc_threshold, sc_min_freq, sc_tht_ssim, sc_min_int, sc_tht_offset)     # raises for the SSIM filter (vsscdect.py:227-233)
    clip, _ = _as_clip(clip)
    ctx = None                                                                                   # the early returns touch no pixel and need no context
    if branch in ("custom", "plugin"):
        ctx = clip.ctx if is_device(clip) else get_context(device_index)
    return scdetect.scene_detect(ctx, clip, threshold=sc_threshold, frequency=sc_min_freq, sc_tht_filter=sc_tht_ssim, min_length=sc_min_int,
                                 tht_white=sc_tht_white, tht_black=sc_tht_black, frame_norm=sc_normalize, tht_offset=sc_tht_offset,
                                 coeffs=scdetect.LUMA_LIMITED if luma_range == "limited" else scdetect.LUMA_FULL)


# ---- HAVC_SceneDetectEdges (vsdeoldify/__init__.py:3227-3258 -> vsslib/vsscdetect_edge.py) ---------------------------------------------------------------
def HAVC_SceneDetectEdges(clip, sc_threshold=0.035, sc_tht_offset=2, sc_tht_ssim=0.80, sc_min_int=20, sc_mult_tht=15, sc_tht_white=0.70, sc_tht_black=0.10,
                          sc_debug=False, *, device_index=0, luma_range="limited"):
    """vsdeoldify/__init__.py:3227-3258: the scene-change frames of a clip by the reference's edge-masked detector, the one it recommends for blended and
    smooth transitions.  The props come back as a `scdetect_edge.EdgeSceneInfo` (a SceneInfo with sc_reason; sc_ratio is zeros), accepted wherever
    `scenes=` is.  The per-frame statistics are ONE launch over the small clip (havc_scene_edge_stats, csrc/scedge.hip); with sc_tht_ssim > 0 (the default)
    the SSIM / histogram filter follows: one havc_scene_hist and one havc_scene_ssim launch over the detector's candidates.  A DeviceImage stays in HBM and
    only per-frame records and scores come back; the decisions are scdetect_edge.edge_detector / edge_scene_filter, on the host.  sc_threshold == 0 flags
    nothing (the reference's early return).  sc_debug is accepted and ignored.  luma_range as in HAVC_SceneDetect."""
    from . import scdetect, scdetect_edge
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_SceneDetectEdges: this is not a clip")
    if luma_range not in ("limited", "full"):
        raise HAVCError("HAVC_SceneDetectEdges: luma_range must be 'limited' or 'full'")
    clip, _ = _as_clip(clip)
    ctx = None                                                                                   # the early return touches no pixel and needs no context
    if scdetect_edge.edges_branch(sc_threshold, 0) == "detect":
        try:
            scdetect_edge.edges_offset(sc_tht_offset, clip.shape[0])
        except ValueError as e:
            raise HAVCError("HAVC_SceneDetectEdges: " + str(e)) from None
        ctx = clip.ctx if is_device(clip) else get_context(device_index)
    return scdetect_edge.scene_detect_edges(ctx, clip, threshold=sc_threshold, frequency=0, ssim_threshold=sc_tht_ssim, sc_diff_offset=sc_tht_offset,
                                            sc_min_int=sc_min_int, sc_mult_tht=sc_mult_tht, tht_white=sc_tht_white, tht_black=sc_tht_black,
                                            coeffs=scdetect.LUMA_LIMITED if luma_range == "limited" else scdetect.LUMA_FULL)


# ---- HAVC_extract_reference_frames / HAVC_export_reference_frames / HAVC_export_list_frames (vsdeoldify/__init__.py:3272-3416 -> vsslib/vsutils.py:147-233) ----
DEF_EXPORT_FORMAT, DEF_JPG_QUALITY = 'jpg', 95                                                     # vsslib/constants.py:58-59


def _export_checks(what, clip, sc_framedir, ref_ext):
    """what touches no pixel, before a context exists -> the extension as the writer uses it (vsutils.py:150: lower case).  Pillow picks the format by the
    file name (everything but "jpg" goes through a bare img.save): an extension it does not know is refused here, where the reference would fail on its
    first frame."""
    from PIL import Image
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError(f"{what}: this is not a clip")
    if not isinstance(sc_framedir, (str, os.PathLike)):
        raise HAVCError(f"{what}: sc_framedir must be a directory name")
    ext = str(ref_ext).lower()
    if "." + ext not in Image.registered_extensions():
        raise HAVCError(f"{what}: Pillow knows no image format for the extension '{ref_ext}'")
    return ext


def _save_ref_frames(clip, frames, numbers, sc_framedir, ext, ref_jpg_quality, ref_override):
    """save_sc_frame (vsutils.py:154-175 / :198-218): frame frames[i] of the clip -> sc_framedir/ref_{numbers[i]:06d}.ext; with ref_override off an
    existing file is left alone.  A DeviceImage clip hands over the listed frames only, one at a time.  -> the paths written"""
    from PIL import Image
    written = []
    for f, num in zip(frames, numbers):
        path = os.path.join(sc_framedir, f"ref_{num:06d}.{ext}")
        if not ref_override and os.path.exists(path):
            continue
        img = Image.fromarray(clip.frame(f).numpy() if is_device(clip) else np.ascontiguousarray(clip[f]), 'RGB')
        if ext == "jpg":
            img.save(path, subsampling=0, quality=ref_jpg_quality)
        else:
            img.save(path)
        written.append(path)
    return written


def _export_scene_frames(clip, scenes, sc_framedir, ref_offset, ext, ref_jpg_quality, ref_override, sequence):
    """vs_sc_export_frames (vsutils.py:147-182): frame 0 and every frame with _SceneChangePrev == 1, named by its number + ref_offset, or with `sequence` by a
    counter from 0 (no offset there) that also counts a frame ref_override leaves alone"""
    frames = [i for i in range(clip.shape[0]) if i == 0 or scenes.scene_change_prev[i] == 1]
    numbers = list(range(len(frames))) if sequence else [i + ref_offset for i in frames]
    return _save_ref_frames(clip, frames, numbers, sc_framedir, ext, ref_jpg_quality, ref_override)


def HAVC_extract_reference_frames(clip, sc_threshold=0.10, sc_tht_offset=1, sc_tht_ssim=0.0, sc_min_int=1, sc_min_freq=0, sc_framedir="./", sc_sequence=False,
                                  sc_normalize=False, ref_offset=0, sc_tht_white=0.70, sc_tht_black=0.10, ref_ext=DEF_EXPORT_FORMAT,
                                  ref_jpg_quality=DEF_JPG_QUALITY, ref_override=True, sc_algo=0, sc_debug=False, *, device_index=0, luma_range="limited",
                                  debug=None):
    """vsdeoldify/__init__.py:3272-3351: detect the scene changes of a clip and write frame 0 and every flagged frame to sc_framedir as ref_nnnnnn.jpg|png --
    the stills HAVC_DeepRemaster(ref_dir=...) reads back once they are coloured.  sc_algo 0 only (SceneDetect + the SSIM filter); the other algorithms are
    VapourSynth plugins.  With 0 < sc_tht_ssim < 1 or sc_min_int > 1 the detection is scdetect.scene_detect_filtered (the SSIM / histogram post-filter: two
    launches over the candidates, csrc/scfilter.hip, the decision on the host), otherwise scdetect.scene_detect as in HAVC_SceneDetect.  The reference returns
    the clip with its props; arrays carry none: the `scdetect.SceneInfo` comes back.  A DeviceImage clip stays in HBM, only the written frames leave it.
    sc_debug is accepted and ignored; `debug` (a dict) receives "written" (the paths) and, with the filter, scene_detect_filtered's launch counts and the
    per-candidate "scores" {frame: (ssim_score, hist_score)}."""
    from . import scdetect
    what = "HAVC_extract_reference_frames"
    ext = _export_checks(what, clip, sc_framedir, ref_ext)
    if luma_range not in ("limited", "full"):
        raise HAVCError(f"{what}: luma_range must be 'limited' or 'full'")
    if sc_algo in (1, 2, 3):
        plugin = {1: "SceneDetectEdges needs the TCanny and akarin plugins", 2: "vs_sc_xvid needs the SCXvid plugin", 3: "vs_mv_sc_detect needs the MVTools plugin"}
        raise NotImplementedError(f"{what}: sc_algo = {sc_algo} is not built ({plugin[sc_algo]}): only sc_algo = 0 (SceneDetect + SSIM filter) is")
    if sc_algo != 0:
        raise HAVCError(f"{what}: sc_algo must be in range [0-3]")
    clip, _ = _as_clip(clip)
    n, h, w, _ = clip.shape
    early = (sc_threshold == 0 and sc_min_freq == 0) or sc_min_freq == 1 or (sc_threshold == 0 and sc_min_freq > 1)      # vsscdect.py:50, 71: no pixel is read
    filtered = not early and scdetect.filter_active(sc_tht_ssim, sc_min_int)
    if filtered and sc_tht_ssim != 1 and min(scdetect.resize_min_hw(w, h)) < scdetect.SSIM_WIN:
        raise HAVCError(f"{what}: the SSIM filter's 7 x 7 window needs frames of at least 7 x 7 (skimage raises below), not {h} x {w}")
    os.makedirs(sc_framedir, exist_ok=True)
    ctx = None if early else (clip.ctx if is_device(clip) else get_context(device_index))
    kw = dict(threshold=sc_threshold, frequency=sc_min_freq, sc_tht_filter=sc_tht_ssim, min_length=sc_min_int, tht_white=sc_tht_white, tht_black=sc_tht_black,
              frame_norm=sc_normalize, tht_offset=sc_tht_offset, coeffs=scdetect.LUMA_LIMITED if luma_range == "limited" else scdetect.LUMA_FULL)
    if filtered:
        scenes = scdetect.scene_detect_filtered(ctx, clip, debug=debug, **kw)
    else:
        scenes = scdetect.scene_detect(ctx, clip, **dict(kw, min_length=1))                     # sc_min_int clamps to 1 here, or an early return ignores it
    written = _export_scene_frames(clip, scenes, sc_framedir, ref_offset, ext, ref_jpg_quality, ref_override, sc_sequence)
    if debug is not None:
        debug["written"] = written
    return scenes


def HAVC_export_reference_frames(clip, sc_framedir="./", ref_offset=0, ref_ext=DEF_EXPORT_FORMAT, ref_jpg_quality=DEF_JPG_QUALITY, ref_override=True, *,
                                 scenes=None, debug=None):
    """vsdeoldify/__init__.py:3364-3385: the writer of HAVC_extract_reference_frames on scene changes that are already known.  The reference reads them off
    the clip's frame props; arrays carry none: `scenes` is the SceneInfo (HAVC_SceneDetect's or HAVC_extract_reference_frames' result for this clip).
    -> the clip, as it came."""
    what = "HAVC_export_reference_frames"
    ext = _export_checks(what, clip, sc_framedir, ref_ext)
    c, _ = _as_clip(clip)
    if scenes is None or len(scenes.scene_change_prev) != c.shape[0]:
        raise HAVCError(f"{what}: scenes= must be the SceneInfo of this clip (the reference reads _SceneChangePrev off every frame)")
    os.makedirs(sc_framedir, exist_ok=True)
    written = _export_scene_frames(c, scenes, sc_framedir, ref_offset, ext, ref_jpg_quality, ref_override, False)
    if debug is not None:
        debug["written"] = written
    return clip


def HAVC_export_list_frames(clip, sc_framedir="./", ref_list=None, offset=0, ref_ext=DEF_EXPORT_FORMAT, ref_jpg_quality=DEF_JPG_QUALITY, ref_override=True,
                            fast_extract=True, *, debug=None):
    """vsdeoldify/__init__.py:3387-3416 -> vs_list_export_frames (vsutils.py:185-233): write the listed frames as ref_nnnnnn.  A list of ONE number k means
    every k-th frame from 0; otherwise the list is sorted and its duplicates dropped.  offset > 0 is added to every number, and the frame that is written
    (and named) is the one at number + offset.  fast_extract picks the frames directly and refuses a number outside the clip; without it the whole clip is
    walked and such a number is never met.  None or an empty list: nothing happens.  -> the clip, as it came."""
    what = "HAVC_export_list_frames"
    if ref_list is None or len(ref_list) < 1:
        return clip
    ext = _export_checks(what, clip, sc_framedir, ref_ext)
    c, _ = _as_clip(clip)
    n = c.shape[0]
    if len(ref_list) == 1:
        if int(ref_list[0]) < 1:
            raise HAVCError(f"{what}: a one-element ref_list is a step and must be positive")
        frames = list(range(0, n, int(ref_list[0])))
    else:
        frames = sorted(set(int(f) for f in ref_list))
    if offset > 0:
        frames = [f + offset for f in frames]
    if fast_extract:
        if any(f < 0 or f > n - 1 for f in frames):
            raise HAVCError("Frame numbers in list must be in range [0, clip.num_frames - 1]")                      # vsutils.py:133-134
    else:
        frames = [f for f in frames if 0 <= f < n]
    os.makedirs(sc_framedir, exist_ok=True)
    written = _save_ref_frames(c, frames, frames, sc_framedir, ext, ref_jpg_quality, ref_override)
    if debug is not None:
        debug["written"] = written
    return clip


# ---- HAVC_deepex (vsdeoldify/__init__.py:1421-1735), ex_model 0 = ColorMNet, method 0 = reference frames from clip_ref -------------------------------------
_REFMERGE_WEIGHT = [0.0, 0.3, 0.4, 0.5, 0.6, 0.7]                                                  # __init__.py:1631


def _deepex_checks(clip, clip_ref, method, ref_merge, sc_framedir, only_ref_frames, ex_model, encode_mode, scenes):
    """the reference's argument checks in its order (__init__.py:1540-1590) as HAVCError, then what this library refuses, each with its reason"""
    def bad(msg):
        raise HAVCError(msg)
    if only_ref_frames and sc_framedir is None:
        bad("HAVC_deepex: only_ref_frames is enabled but sc_framedir is unset")
    if sc_framedir is not None and method != 0 and only_ref_frames:
        bad("HAVC_deepex: only_ref_frames is enabled but method != 0 (HAVC)")
    if method != 0 and sc_framedir is None:
        bad("HAVC_deepex: method != 0 but sc_framedir is unset")
    if method in (3, 4) and clip_ref is not None:
        bad("HAVC_deepex: method in (3, 4) but clip_ref is set")
    if method in (0, 1, 2, 5, 6) and clip_ref is None:
        bad("HAVC_deepex: method in (0, 1, 2, 5, 6) but clip_ref is unset")
    if clip_ref is not None and not (is_device(clip_ref) or isinstance(clip_ref, np.ndarray)):
        bad("HAVC_deepex: this is not a clip: clip_ref")
    if method not in range(7):
        bad("HAVC_deepex: method must be in range [0-6]")
    if ref_merge not in range(6):
        bad("HAVC_deepex: ref_merge must be in range [0-5]")
    if ref_merge > 0 and (method not in (0, 1, 5) and ex_model != 3):
        bad("HAVC_deepex: method must be in (0, 1, 5) to be used with ref_merge > 0")
    if method in (0, 1, 2):
        # get_sc_props(clip_ref): arrays carry no frame props, `scenes` is what the reference reads off clip_ref; no props = (0, 0) there (vsscdect.py:104-115)
        sc_threshold, sc_frequency = (scenes.sc_threshold, scenes.sc_frequency) if scenes is not None else (0, 0)
        if sc_threshold == 0 and sc_frequency == 0:
            bad("HAVC_deepex: method in (0, 1, 2) but sc_threshold and sc_frequency are not set")
        if sc_frequency == 1 and only_ref_frames:
            bad("HAVC_deepex: only_ref_frames is enabled but sc_frequency == 1 or ColorTemp/FrameInterp are set ")
        if not only_ref_frames and ref_merge > 0 and sc_frequency != 1 and ex_model != 3:
            bad("HAVC_deepex: method in (0, 1, 2) and ref_merge > 0 but sc_frequency != 1")
    if method in (0, 1, 2) and ex_model == 2:
        bad("HAVC_deepex: DeepRemaster cannot be used with methods: 0, 1, 2 (HAVC)")
    if ex_model in (1, 2, 3):
        raise NotImplementedError("HAVC_deepex: ex_model 1-3 (Deep-Exemplar, DeepRemaster, Deep-CMnet) are not built: only ColorMNet (ex_model = 0) is, DESIGN.md section 7")
    if ex_model != 0:
        bad("HybridAVC: unknown exemplar model id: " + str(ex_model))                             # __init__.py:1724
    if method != 0:
        raise NotImplementedError("HAVC_deepex: methods 1-6 take their reference frames from a directory or a video (sc_framedir, HAVC_restore_video): "
                                  "only method 0 (reference frames from clip_ref) is built")
    if sc_framedir is not None or only_ref_frames:
        raise NotImplementedError("HAVC_deepex: sc_framedir / only_ref_frames write the reference frames to files: not in this harness")
    if encode_mode == 2:
        raise NotImplementedError("HAVC_deepex: encode_mode = 2 is not built; 0 and 1 both run in process, as DeepExColorMNet does")
    if encode_mode not in (0, 1):
        bad("HAVC_deepex: encode_mode must be 0, 1 or 2")


def HAVC_deepex(clip=None, clip_ref=None, method=0, render_speed='medium', render_vivid=True, ref_merge=0, sc_framedir=None, ref_norm=False,
                only_ref_frames=False, dark=False, dark_p=(0.2, 0.8), smooth=False, smooth_p=(0.3, 0.7, 0.9, 0.0, "none"), colormap="none",
                ref_weight=None, ref_thresh=None, ref_freq=None, ex_model=0, encode_mode=0, max_memory_frames=0, torch_dir=None, *, scenes=None, **harness):
    """vsdeoldify/__init__.py:1421-1735 with ex_model = 0 (ColorMNet) and method = 0 (reference frames from clip_ref, e.g. HAVC_colorizer's output): every
    frame `scenes` flags (and frame 0) hands its clip_ref frame to ColorMNet as the new reference, the others are propagated.  `scenes` is the SceneInfo the
    reference reads off clip_ref's frame props (get_sc_props, CopySCDetect): HAVC_SceneDetect's result for the clip clip_ref was made of.  ref_merge > 0 (with
    scenes.sc_frequency == 1: every frame has a reference) detects the scenes of `clip` itself (threshold ref_thresh, frequency ref_freq, ref_norm) and merges
    every frame that is no scene change with its squashed reference frame at weight ref_weight (default [0, .3, .4, .5, .6, .7][ref_merge]).  colormap ->
    dark -> smooth are applied to the squashed reference frames that are scene changes (vs_sc_*: vsfilters.py:525-636), one launch (havc_stabilizer_chain); a
    colormap NAME goes through _get_colormap as in HAVC_stabilizer (the reference hands the bare name to image_chroma_tweak, where its parser raises).
    ndarray in -> ndarray out; a DeviceImage clip (and clip_ref) stays in HBM end to end.  Frames go through DeepExColorMNet.colorize_frame one by one.
    `harness` = keyword-only extras of this library: state_dict / network (seeded ColorMNet weights or a built ColorMNetNetwork instead of the files under
    torch_dir), device_index, luma_range (HAVC_SceneDetect's), debug (a dict that receives "ref_small": the squashed, tweaked reference frames by index,
    "clip_sc": the SceneInfo of clip, "ref_weight")."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_deepex: this is not a clip")
    unknown = set(harness) - {"state_dict", "network", "device_index", "luma_range", "debug"}
    if unknown:
        raise TypeError(f"HAVC_deepex: unexpected keyword arguments {sorted(unknown)}")
    if not isinstance(render_speed, str) or not isinstance(colormap, str):
        raise HAVCError("HAVC_deepex: render_speed and colormap must be strings")
    _deepex_checks(clip, clip_ref, method, ref_merge, sc_framedir, only_ref_frames, ex_model, encode_mode, scenes)
    from .colormnet_render import DEEPEX_SIZES
    if render_speed.lower() not in DEEPEX_SIZES:
        raise HAVCError("HAVC_deepex: unknown render_speed ->" + render_speed)                     # deepex/__init__.py:50-83
    dark_args = smooth_args = None                                                                # __init__.py:1606-1628
    if dark:
        dark_args = (dark_p[0], dark_p[1], (dark_p[2] if len(dark_p) > 2 else "none").lower())
    if smooth:
        smooth_args = (smooth_p[0], smooth_p[1], smooth_p[2], -smooth_p[3], (smooth_p[4] if len(smooth_p) > 4 else "none").lower())
    colormap = colormap.lower()
    colormap_adjust = _get_colormap(colormap) if colormap not in ("none", "") else None
    if colormap_adjust is not None:
        try:
            F.parse_hue_ranges(F.parse_hue_adjust(colormap_adjust)[0])
        except ValueError:
            raise HAVCError("HAVC_main: ColorMap choice is invalid for '" + colormap + "'") from None
    clip, single = _as_clip(clip)
    clip_ref, _ = _as_clip(clip_ref)
    n = clip.shape[0]
    if tuple(clip_ref.shape) != tuple(clip.shape):
        raise HAVCError(f"HAVC_deepex: clip_ref {tuple(clip_ref.shape)} must have the frames and the size of clip {tuple(clip.shape)}")
    for f in ("scene_change_prev", "scene_change_next"):
        if len(getattr(scenes, f)) != n:
            raise HAVCError(f"HAVC_deepex: scenes.{f} has {len(getattr(scenes, f))} entries for a clip of {n} frames")
    # ---- everything below touches the GPU ----
    from . import scdetect
    from .colormnet_render import DeepExColorMNet
    from .stabilizer import stabilize_np
    enable_refmerge = ref_merge > 0 and scenes.sc_frequency == 1                                  # __init__.py:1630-1645
    if max_memory_frames > 0:
        render_vivid = False                                                                      # __init__.py:1692-1693: HAVC_deepex alone, not HAVC_restore_video
    dx = DeepExColorMNet(vid_length=n, render_speed=render_speed, enable_resize=False, render_vivid=render_vivid, max_memory_frames=max_memory_frames,
                         frame_propagate=False, project_dir=torch_dir, state_dict=harness.get("state_dict"), device_index=harness.get("device_index", 0),
                         network=harness.get("network"))
    ctx = dx.ctx
    clip_sc = None
    if enable_refmerge:
        if ref_weight is None:
            ref_weight = _REFMERGE_WEIGHT[ref_merge]
        if ref_thresh is None:
            ref_thresh = scdetect.DEF_THRESHOLD
        if ref_freq is None or ref_freq == 1:
            ref_freq = 0
        coeffs = scdetect.LUMA_FULL if harness.get("luma_range", "limited") == "full" else scdetect.LUMA_LIMITED
        clip_sc = scdetect.scene_detect(ctx, clip, threshold=ref_thresh, frequency=ref_freq, frame_norm=ref_norm, coeffs=coeffs)
    else:
        ref_weight = 1.0
    tweak = None
    if dark_args or smooth_args or colormap_adjust:
        def tweak(sq):
            return stabilize_np(ctx, sq, dark_args, smooth_args, colormap_adjust, order=("colormap", "dark", "smooth"))            # __init__.py:1679-1689
    return _colormnet_clip(dx, clip, clip_ref, scenes, clip_sc, ref_weight, single, tweak, harness.get("debug"))


def _colormnet_clip(dx, clip, clip_ref, scenes, clip_sc, ref_weight, single, tweak=None, debug=None):
    """vs_colormnet's frame loop (colormnet/__init__.py) on 4-D operands, shared by HAVC_deepex and HAVC_restore_video: every frame `scenes` flags (and
    frame 0) hands its clip_ref frame to ColorMNet as the new reference; with 0 < ref_weight < 1 and a clip_sc the flags come from clip_sc instead and
    every frame that is no scene change is blended with its squashed reference frame.  tweak: applied to the squashed reference frames that `scenes`
    flags (HAVC_deepex's colormap / dark / smooth)."""
    ctx = dx.ctx
    n = clip.shape[0]
    host_in = not is_device(clip)
    dclip = DeviceImage.from_numpy(ctx, clip) if host_in else clip
    dref = clip_ref if is_device(clip_ref) else DeviceImage.from_numpy(ctx, clip_ref)
    merging = 0 < ref_weight < 1 and clip_sc is not None                                          # colormnet/__init__.py:135
    flags = clip_sc if merging else scenes                                                        # f[2] there, f[1] otherwise
    ref_small = {}

    def small_ref(i):
        """clip_ref's frame i at the DeepEx size (SmartResizeReference), tweaked where clip_ref's own props make it a scene change (vs_sc_*)"""
        if i not in ref_small:
            sq, _ = dx._squash(dref.frame(i))
            if (i == 0 or scenes.scene_change_prev[i] == 1) and tweak is not None:
                sq = tweak(sq)
            ref_small[i] = sq
        return ref_small[i]

    out = DeviceImage(ctx, dclip.shape)
    for i in range(n):
        is_sc = flags.scene_change_prev[i] == 1
        col = dx.colorize_frame(dclip.frame(i), ref_small=small_ref(i) if (i == 0 or is_sc) else None,
                                blend=(small_ref(i), ref_weight) if (merging and not is_sc) else None)
        col = col if is_device(col) else DeviceImage.from_numpy(ctx, np.ascontiguousarray(col))  # (the border path of DeepExColorMNet finishes on the host)
        out.frame(i).copy_from(col)
        if debug is None:
            ref_small.pop(i, None)
    if debug is not None:
        debug.update(ref_small=dict(ref_small), clip_sc=clip_sc, ref_weight=ref_weight)
    if host_in:
        out = out.numpy()
        return out[0] if single else out
    return out.reshaped(out.shape[1:]) if single else out


# ---- HAVC_bw_tune (vsdeoldify/__init__.py:1266-1339) / HAVC_auto_levels (:3150-3179 -> havc_utils.vs_auto_levels, havc_utils.py:785-833) ---------------------
_BW_TUNE = ['none', 'light', 'medium', 'strong']                                                   # __init__.py:1294, havc_utils.py:813


def _bw_tune_id(name):
    if not isinstance(name, str):
        raise HAVCError("HAVC_bw_tune: B&W tune choice must be a string")
    try:
        return _BW_TUNE.index(name.lower())
    except ValueError:                                                                            # HAVC_LogMessage joins its arguments with a blank
        raise HAVCError("HAVC_bw_tune: B&W tune choice is invalid:  " + name.lower()) from None


def _equalize_clip(clip, device_index, **kw):
    """a checked clip through equalize.rgb_equalizer_np; the refusals of check_args come before the context exists"""
    from . import equalize
    clip, single = _as_clip(clip)
    equalize.check_args(clip.shape, kw["method"])
    ctx = clip.ctx if is_device(clip) else get_context(device_index)
    if kw.pop("range_tv_tables"):                                                                 # __init__.py:1324-1326, 1335-1337
        kw.update(lut_in=equalize.tv_in_table(), lut_out=equalize.tv_out_table())
    out = equalize.rgb_equalizer_np(ctx, clip, **kw)
    if single:
        return out.reshaped(out.shape[1:]) if is_device(out) else out[0]
    return out


def HAVC_auto_levels(clip=None, mode='Light', method=0, luma_blend=False, range_tv=True, *, device_index=0):
    """vsdeoldify/__init__.py:3150-3179: histogram equalisation (auto levels) as a pre-filter for dark B&W clips -- rgb_equalizer with strength 0.98 / 0.99 /
    1.0 ('Light' / 'Medium' / 'Strong'; 'None' = 0: only the range round trip is left), clip_limit 1.0, weight3 0.3, between the range conversions when
    range_tv.  One havc_equalize_clip call: two launches over the whole clip.  ndarray in -> ndarray out; DeviceImage in -> DeviceImage out (nothing
    leaves HBM, the call only enqueues).  Methods 4 and 5 are refused."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_bw_tune: this is not a clip")                                       # havc_utils.py:809-810 (the text names HAVC_bw_tune there)
    bw_id = _bw_tune_id(mode)                                                                     # havc_utils.py:812-820
    b_strength = [0.0, 0.98, 0.99, 1.0]
    return _equalize_clip(clip, device_index, method=method, strength=b_strength[bw_id], luma_blend=luma_blend, range_tv=range_tv,
                          range_tv_tables=bool(range_tv))


def HAVC_bw_tune(clip=None, bw_tune='Light', bw_method=0, luma_blend=True, range_tv=True, chroma_resize=False, *, device_index=0):
    """vsdeoldify/__init__.py:1266-1339: the contrast / colour stage every HAVC_main preset ends in -- rgb_balance (per-channel gains from the channel
    means, rgb_factor and strength by tune) and rgb_equalizer (method bw_method, strength 0.30 / 0.40 / 0.50) between the range conversions when range_tv.
    One havc_equalize_clip call: three launches over the whole clip.  'None' returns the clip.  ndarray in -> ndarray out; DeviceImage in -> DeviceImage
    out (nothing leaves HBM, the call only enqueues).  Methods 4 and 5 and chroma_resize=True are refused."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_bw_tune: this is not a clip")
    if chroma_resize:                                                                             # __init__.py:1291 -> havc_utils.py:57-140
        raise NotImplementedError("HAVC_bw_tune(chroma_resize=True): the downscale is a zimg round trip inside convert_format_RGB24 / restore_format "
                                  "(havc_utils.py:57-140): not in this harness")
    bw_id = _bw_tune_id(bw_tune)                                                                  # __init__.py:1293-1310
    b_strength = [0.0, 0.30, 0.40, 0.50]
    w_strength = [0.0, 0.30, 0.40, 0.50]
    r_factor, g_factor, b_factor = [1.0, 0.96, 0.94, 0.92], [1.0, 1.03, 1.05, 1.08], [1.0, 1.0, 1.0, 1.0]
    bw_method = min(5, bw_method)                                                                 # :1301
    if bw_id == 0:                                                                                # :1312-1313
        return clip
    return _equalize_clip(clip, device_index, method=bw_method, strength=b_strength[bw_id], weight3=w_strength[bw_id], luma_blend=luma_blend,
                          range_tv=range_tv, range_tv_tables=bool(range_tv),
                          balance=(w_strength[bw_id], [r_factor[bw_id], g_factor[bw_id], b_factor[bw_id]]))       # :1328-1333


# ---- HAVC_retinex (vsdeoldify/__init__.py:1073-1101 -> vsslib/vsretinex.py:25-88 vs_retinex / vs_retinex_fast) ----------------------------------------
def HAVC_retinex(clip, luma_dark=0.20, luma_bright=0.80, sigmas=(25, 80, 250), range_tv_in=True, range_tv_out=True, blend=False, chroma_resize=False, *,
                 device_index=0):
    """vsdeoldify/__init__.py:1073-1101: multi-scale Retinex (MSRCP) that leaves dark and bright frames alone -- a frame whose f_luma lies outside
    [luma_dark, luma_bright] comes back as it went in; with blend the result of a frame below 0.40 is blended over the input.  The plugin's pixel work is
    a stand-in restated from its published algorithm (retinex.py says what is pinned and what is not).  One havc_retinex_clip call: seven launches per
    chunk of frames, float64 Gaussians.  A frame or a clip; ndarray in -> ndarray out; DeviceImage in -> DeviceImage out (nothing leaves HBM, the call
    only enqueues).  chroma_resize=True is refused."""
    from . import retinex
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_retinex: this is not a clip")
    retinex.check_args(tuple(clip.shape), sigmas, chroma_resize, clip.dtype if isinstance(clip, np.ndarray) else np.uint8)
    clip, single = _as_clip(clip)
    ctx = clip.ctx if is_device(clip) else get_context(device_index)
    out = retinex.retinex_np(ctx, clip, **retinex.plugin_args(sigmas, range_tv_in, range_tv_out),                       # vsretinex.py:58-59
                             luma_dark=luma_dark, luma_bright=luma_bright, range_tv=range_tv_in, blend=blend)          # :86-87
    if single:
        return out.reshaped(out.shape[1:]) if is_device(out) else out[0]
    return out


# ---- HAVC_tweak / HAVC_adjust_rgb / HAVC_rgb_denoise (vsdeoldify/__init__.py:1377-1408, 1342-1374, 924-944) ----------------------------------------------
def _is_clip(clip):
    return clip is not None and (is_device(clip) or isinstance(clip, np.ndarray))


def HAVC_tweak(clip=None, hue=0, sat=1, bright=0, cont=1, gamma=1, *, device_index=0):
    """vsdeoldify/__init__.py:1377-1408 -> vs_tweak: hue (degrees), saturation, brightness (-1 < bright < 1 is scaled by 255), contrast and gamma of an RGB24
    clip, through YUV420P8 (BT.709, full range) and back with error diffusion.  The two conversions are a stand-in for zimg with one written definition
    (tweak.py says what is pinned and what is not); the kernels equal it byte for byte.  The neutral call returns the clip.  One havc_tweak_clip call: two
    launches per chunk of frames.  A frame or a clip; ndarray in -> ndarray out; DeviceImage in -> DeviceImage out (nothing leaves HBM, the call only
    enqueues).  An odd width or height (VapourSynth refuses YUV420 there) and gamma <= 0 are refused.  The vs_tweak refusals inside HAVC_colorizer,
    HAVC_DeepRemaster, HAVC_restore_video and ddtweak stay: routing them here is a separate decision."""
    from . import tweak
    if not _is_clip(clip):
        raise HAVCError("HAVC_tweak: this is not a clip")
    tweak.check_clip(tuple(clip.shape), clip.dtype if isinstance(clip, np.ndarray) else np.uint8, "HAVC_tweak", True)
    if not gamma > 0:
        raise HAVCError(f"HAVC_tweak: gamma = {gamma}: std.Levels needs gamma > 0")
    plan = tweak.tweak_plan(hue, sat, bright, cont, gamma)
    if plan is None:                                                                              # vsfilters.py:781-782
        return clip
    ctx = clip.ctx if is_device(clip) else get_context(device_index)
    return tweak.tweak_np(ctx, clip, plan)


def HAVC_adjust_rgb(clip=None, strength=0.0, factor=(1.0, 1.0, 1.0), bias=(0, 0, 0), gamma=(1.0, 1.0, 1.0), *, device_index=0, color_range=None):
    """vsdeoldify/__init__.py:1342-1374: grey-world normalisation of every frame (vs_rgb_normalize; strength 1 = all of it, 0 < strength < 1 = std.Merge by
    strength, anything else = none), then per channel x * factor + bias and gamma (adjust_rgb).  Every stage is a function of the sample and the frame's
    channel means: the library composes 3 x 256 bytes per frame on the device and applies them in one pass (three launches, nothing read back).
    color_range: the reference asks the clip's range prop and an array has none -- None and "limited" take its limited branch, which is also what it does
    to a clip without the prop (a bias is scaled by 256 / 235 and must lie in [-235, 235]); "full": 256 / 255 and [-255, 255].  A frame or a clip; ndarray
    in -> ndarray out; DeviceImage in -> DeviceImage out (the call only enqueues)."""
    from . import tweak
    if not _is_clip(clip):
        raise HAVCError("HAVC_adjust_rgb: this is not a clip")
    tweak.check_clip(tuple(clip.shape), clip.dtype if isinstance(clip, np.ndarray) else np.uint8, "HAVC_adjust_rgb", False)
    plan = tweak.adjust_plan(factor, bias, gamma, color_range)
    ctx = clip.ctx if is_device(clip) else get_context(device_index)
    return tweak.adjust_rgb_np(ctx, clip, strength, plan)


def HAVC_rgb_denoise(clip=None, denoise_levels=(0.4, 0.3), rgb_factors=(0.95, 1.05, 1.01), *, device_index=0):
    """vsdeoldify/__init__.py:924-944 -> rgb_denoise (havc_utils.py:752-773): colour post-process for DDColor / Zhang clips -- between the TV-range
    conversions, rgb_balance(strength = denoise_levels[0], rgb_factors) and rgb_equalizer(method 0 = CLAHE on luma, strength = denoise_levels[1],
    luma_blend off, range_tv on).  One havc_equalize_clip call, three launches; frames of at least 8 x 8.  ndarray in -> ndarray out; DeviceImage in ->
    DeviceImage out (the call only enqueues)."""
    if not _is_clip(clip):
        raise HAVCError("HAVC_rgb_denoise: this is not a clip")
    from . import tweak
    tweak.check_clip(tuple(clip.shape), clip.dtype if isinstance(clip, np.ndarray) else np.uint8, "HAVC_rgb_denoise", False)
    return _equalize_clip(clip, device_index, method=0, strength=denoise_levels[1], luma_blend=False, range_tv=True, range_tv_tables=True,
                          balance=(denoise_levels[0], [rgb_factors[0], rgb_factors[1], rgb_factors[2]]))


# ---- HAVC_TimeCube / HAVC_clip_overlay (vsdeoldify/__init__.py:2995-3026, 3029-3148) ----------------------------------------------------------------------
def HAVC_TimeCube(clip, strength=1.0, lut_effect=0, factors=None, *, lut_dir=None, cube=None, device_index=0):
    """vsdeoldify/__init__.py:2995-3026 -> vs_timecube (vsslib/vsplugins.py:325-378): the 3D LUT of `lut_effect` (0..11: the twelve .cube files under
    <lut_dir>/color/), vs_tweak with the effect's hue / sat / bright / cont / gamma (or `factors`, those five in that order), then a merge with the input by
    `strength`: std.Merge, or for effect 8 ChromaBoundAdaptiveMerge (combine_models method 7, cmc_p [0.15, True, 25, 25]).  strength 0 returns the clip itself,
    strength 1 skips the merge.  Keyword-only extras of this library: lut_dir (default: the environment variable HAVC_LUT_DIR), and cube -- a path or a
    timecube.Cube that replaces the file lookup while lut_effect still selects the factors and the merge.  The timecube.Cube plugin is a stand-in with one
    written definition (timecube.py says what is pinned and what is not); the kernel equals it byte for byte.  A LUT file that is not there raises HAVCError
    (the reference logs and carries on un-graded).  Per call: the LUT (two launches), havc_tweak_clip (two per chunk of frames; not with neutral factors), the
    merge.  With a tweak the frame needs an even width and height; with neutral factors (0, 1, 0, 1, 1) any size passes.  A frame or a clip; ndarray in ->
    ndarray out; DeviceImage in -> DeviceImage out (nothing is read back)."""
    from . import timecube, tweak
    if not _is_clip(clip):
        raise HAVCError("HAVC_TimeCube: this is not a clip")
    tweak.check_clip(tuple(clip.shape), clip.dtype if isinstance(clip, np.ndarray) else np.uint8, "HAVC_TimeCube", False)
    if lut_dir is None:
        lut_dir = os.environ.get("HAVC_LUT_DIR") or None
    plan = timecube.timecube_plan(strength, lut_effect, factors, lut_dir, cube)
    if plan["identity"]:                                                                          # vsplugins.py:327-328
        return clip
    tw = plan["tweak"]
    if not tw["gamma"] > 0:
        raise HAVCError(f"HAVC_TimeCube: gamma = {tw['gamma']}: std.Levels needs gamma > 0")
    tweak_plan = tweak.tweak_plan(**tw)
    if tweak_plan is not None:
        tweak.check_clip(tuple(clip.shape), np.uint8, "HAVC_TimeCube", True)
    lut = timecube.load_cube(plan, cube)
    ctx = clip.ctx if is_device(clip) else get_context(device_index)
    new = timecube.lut3d_np(ctx, clip, lut)
    if tweak_plan is not None:
        new = tweak.tweak_np(ctx, new, tweak_plan)
    if plan["merge"] is None:
        return new
    shape = tuple(clip.shape)
    as4 = (lambda x: x.reshaped((1,) + shape) if len(shape) == 3 else x) if is_device(clip) else (lambda x: x.reshape((-1,) + shape[-3:]))
    a, b = as4(clip if is_device(clip) else np.ascontiguousarray(clip)), as4(new)
    if plan["merge"][0] == "combine_models":
        kw = plan["merge"][1]
        out = combine_models(a, b, kw["method"], kw["w"], cmc_p=kw["cmc_p"], device_index=device_index)
    else:
        out = combine_models(a, b, 2, plan["merge"][1], device_index=device_index)                # vs.core.std.Merge = simple_merge
    return out.reshaped(shape) if is_device(out) else out.reshape(shape)


def HAVC_clip_overlay(base, overlay, x=0, y=0, mask=None, opacity=1.0, mode='normal', planes=None, mask_first_plane=True, *, device_index=0):
    """vsdeoldify/__init__.py:3029-3148 on RGB24 clips: `overlay` ([n, h, w, 3], or one frame [h, w, 3] that is repeated) is put on `base` [n, H, W, 3] with its
    top left corner at (x, y), either sign; the result has the base's shape.  mode: normal, addition, average, difference, divide, exclusion, multiply, overlay,
    subtract.  mask: uint8, the overlay's height and width, gray [n, h, w] or three planes [n, h, w, 3] (plane 0 serves all planes with mask_first_plane), as
    many frames as the overlay; where it is darker the overlay is more transparent.  opacity (clamped to [0, 1]) multiplies the mask.  planes: None (all), an
    int or a list: the others are the base's.  An overlay entirely outside the base returns a copy of the base.  The native filters underneath are a stand-in
    with one written definition (overlay.py); the kernel equals it byte for byte.  One launch; nothing is cropped, padded or read back.  The base decides the
    kind of the result: ndarray -> ndarray, DeviceImage -> DeviceImage; overlay and mask may be of either kind."""
    from . import overlay as ov
    if not (_is_clip(base) and _is_clip(overlay)):
        raise HAVCError('mask_overlay: this is not a clip')
    if mask is not None and not _is_clip(mask):
        raise HAVCError('mask_overlay: mask is not a clip')
    for c in (base, overlay, mask):
        if isinstance(c, np.ndarray) and c.dtype != np.uint8:
            raise HAVCError("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    plan = ov.overlay_plan(base.shape, overlay.shape, None if mask is None else mask.shape, x, y, opacity, mode, planes, mask_first_plane)
    ctx = base.ctx if is_device(base) else get_context(device_index)
    return ov.overlay_np(ctx, base, overlay, mask, plan)


# ---- HAVC_DeepRemaster (vsdeoldify/__init__.py:2689-2735 -> remaster/__init__.py:203-307 vs_remaster_colorize) ----------------------------------------
def HAVC_DeepRemaster(clip, length=2, render_vivid=False, ref_dir=None, ref_minedge=256, frame_mindim=320, ref_buffer_size=20, device_index=0,
                      inference_mode=False, mode=0, *, state_dict=None, model=None, weights_dir=None):
    """DeepRemaster with reference stills from a directory (mode 0): the clip is brought to the inference size (resize_for_inference: the shorter side
    to frame_mindim, both sides to multiples of 16; the library's Spline64 for zimg's), runs through RemasterRender in batches of `length` frames
    (the last batch may be shorter; the window of stills moves with the batch's last frame number), goes back to its size with Spline64 and keeps
    its own luma (vs_recover_resolution = chroma_post_process with the source as luma, fused into the resize).  ndarray in -> ndarray out; a DeviceImage
    clip stays in HBM.  inference_mode is accepted and ignored (a torch switch).  Refused, not approximated: render_vivid=True (vs_tweak: a zimg YUV420
    round trip) and mode=1 (reference frames through VapourSynth clips and scene-change props).  Keyword-only extras of this library: state_dict / model
    (seeded NetworkC weights or a built RemasterColorNet instead of weights_dir/remasternet.pth.tar)."""
    if clip is None or not (is_device(clip) or isinstance(clip, np.ndarray)):
        raise HAVCError("HAVC_DeepRemaster: this is not a clip")
    if ref_dir is None:
        raise HAVCError("HAVC_DeepRemaster: ref_dir is unset")
    if mode != 0:
        raise NotImplementedError("HAVC_DeepRemaster: mode = 1 reads its reference frames through VapourSynth clips and scene-change frame props: only mode = 0 "
                                  "(direct access to the reference frame folder) is built")
    if not os.path.isdir(ref_dir):
        raise HAVCError(f"HAVC_DeepRemaster: '{ref_dir}' is not a valid directory")
    if length < 2:
        raise HAVCError("HAVC_DeepRemaster: length must be at least 2")
    if render_vivid:
        raise NotImplementedError("HAVC_DeepRemaster: render_vivid is vs_tweak (a zimg YUV420 round trip): not in this harness")
    from .remaster_render import RemasterRender, get_ref_list, resize_for_inference_size
    if not get_ref_list(ref_dir)[0]:
        raise HAVCError(f"HAVC_DeepRemaster: no reference frames found in {ref_dir}")
    clip, single = _as_clip(clip)
    n, h, w = clip.shape[0], clip.shape[1], clip.shape[2]
    fw, fh = resize_for_inference_size(w, h, frame_mindim)
    # ---- everything below touches the GPU ----
    engine = RemasterRender(device_index=device_index, ref_minedge=ref_minedge, ref_buffer_size=ref_buffer_size, length=length, model_dir=weights_dir,
                            state_dict=state_dict, model=model)
    try:
        engine.load_ref_dir(ref_dir)
        ctx = engine._ctx()
        host_in = not is_device(clip)
        dclip = DeviceImage.from_numpy(ctx, clip) if host_in else clip
        small = spline64(ctx, dclip, fw, fh)
        colored = DeviceImage(ctx, small.shape)
        for n0 in range(0, n, length):
            n1 = min(n0 + length, n)
            colored.frames(n0, n1).copy_from(engine.process_frames(small.frames(n0, n1), last_frame_idx=min(n0 + length - 1, n - 1)))
        out = spline64(ctx, colored, w, h, luma_from=dclip)
        if host_in:
            out = out.numpy()
            return out[0] if single else out
        ctx.synchronize()
        return out.reshaped(out.shape[1:]) if single else out
    finally:
        engine.close()


# ---- HAVC_restore_video (vsdeoldify/__init__.py:1959-2127) ------------------------------------------------------------------------------------------------
DEF_MIN_FREQ, DEF_NUM_RF_FRAMES = 10, 10                                                           # vsslib/constants.py:61, 66


def restore_video_params(method, ex_model, ref_merge, ref_weight, ref_thresh, ref_freq):
    """the parameter defaulting of __init__.py:2066-2083 -> (ref_thresh, ref_freq, ref_weight, merge): merge = False: the scenes of clip_ref are its
    references, weight 1.0 and no clip_sc; merge = True (method 5 with ref_merge > 0): every clip_ref frame is a reference and clip_sc holds its scenes"""
    from . import scdetect
    if ref_thresh is None or ref_thresh == 0:
        ref_thresh = scdetect.DEF_THRESHOLD
    if ref_freq is None or ref_freq == 0:
        ref_freq = DEF_MIN_FREQ if ex_model == 2 else 0
    if ref_merge == 0 or method in (2, 6):
        return ref_thresh, ref_freq, 1.0, False
    if ref_weight is None or ref_weight == 0:
        ref_weight = _REFMERGE_WEIGHT[ref_merge]
    return ref_thresh, ref_freq, ref_weight, True


def HAVC_restore_video(clip=None, clip_ref=None, method=6, render_speed='medium', ex_model=0, ref_merge=0, ref_weight=None, ref_thresh=None, ref_freq=None,
                       ref_norm=False, max_memory_frames=0, render_vivid=True, encode_mode=0, encode_first=True, torch_dir=None, **harness):
    """vsdeoldify/__init__.py:1959-2127: the colours of a reference VIDEO of the same film (clip_ref: the same frames, any size) moved onto the B&W master
    `clip` with ColorMNet (ex_model 0) or DeepRemaster (ex_model 2).  clip_ref of another size is brought to the clip's with the library's Spline36 (zimg's
    there).  Method 6 (or ref_merge 0): the reference frames are the scene changes of clip_ref (threshold ref_thresh, default 0.10; frequency ref_freq,
    default 10 for DeepRemaster and 0 otherwise; ref_norm).  Method 5 with ref_merge > 0: every clip_ref frame is a reference, the scenes of clip_ref
    become clip_sc, and the frames are blended with their clip_ref frame at ref_weight (default [0, .3, .4, .5, .6, .7][ref_merge]).
    ex_model 0 is HAVC_deepex's ColorMNet loop (no colormap / dark / smooth); render_vivid reaches ColorMNet unchanged (memory reset at every reference
    update), also with max_memory_frames > 0, where HAVC_deepex alone switches it off.  render_speed is checked for every ex_model, as there.  ex_model 2 is vs_deepremaster -> vs_sc_remaster_colorize
    (vsmodels.py:164-178, remaster/__init__.py:40-200): max_memory_frames (default 10, at least 4) stills in the window, batches of 2 frames at the
    inference size (Spline64), the stills taken from clip_ref where clip_sc (or clip_ref's own scenes) flags them (remaster_render.RemasterClipRender);
    with 0 < ref_weight < 1 and a clip_sc EVERY coloured frame is blended with its clip_ref frame (Pillow LANCZOS to the inference size); Spline64 back
    with the clip's luma, and the luma once more (vs_recover_clip_luma, :2125).  ndarray in -> ndarray out; DeviceImage operands stay in HBM.
    encode_first is accepted and ignored (it chooses a second server process there).  Refused, not approximated: ex_model 1 (Deep-Exemplar: not built),
    ex_model 2 with render_vivid=True (vs_tweak: zimg), encode_mode 2.  `harness` = keyword-only extras of this library: state_dict / network (ColorMNet)
    or state_dict / model (DeepRemaster) instead of the weight files, device_index, luma_range (HAVC_SceneDetect's), frame_mindim / ref_minedge
    (DeepRemaster's sizes, 320 / 256 in the reference), debug (a dict that receives "scenes", "clip_sc", "ref_weight", "clip_ref": the resized clip_ref,
    and the ColorMNet loop's "ref_small")."""
    for c in (clip, clip_ref):
        if c is None or not (is_device(c) or isinstance(c, np.ndarray)):
            raise HAVCError("HAVC_restore_video: this is not a clip")
    unknown = set(harness) - {"state_dict", "network", "model", "device_index", "luma_range", "frame_mindim", "ref_minedge", "debug"}
    if unknown:
        raise TypeError(f"HAVC_restore_video: unexpected keyword arguments {sorted(unknown)}")
    if method not in (5, 6):
        raise HAVCError("HAVC: Video restore is supported only with methods: 5, 6")                 # __init__.py:2048
    if ex_model not in (0, 1, 2):
        raise HAVCError("HybridAVC: unknown exemplar model id: " + str(ex_model))                  # :2120
    if ex_model == 1:
        raise NotImplementedError("HAVC_restore_video: ex_model 1 (Deep-Exemplar) is not built: ColorMNet (0) and DeepRemaster (2) are, DESIGN.md section 7")
    if ex_model == 2 and render_vivid:
        raise NotImplementedError("HAVC_restore_video: render_vivid is vs_tweak (a zimg YUV420 round trip): not in this harness")
    if encode_mode == 2:
        raise NotImplementedError("HAVC_restore_video: encode_mode = 2 is not built; 0 and 1 both run in process, as DeepExColorMNet does")
    if encode_mode not in (0, 1):
        raise HAVCError("HAVC_restore_video: encode_mode must be 0, 1 or 2")
    if ref_merge not in range(6):
        raise HAVCError("HAVC_restore_video: ref_merge must be in range [0-5]")
    if not isinstance(render_speed, str):
        raise HAVCError("HAVC_restore_video: render_speed must be a string")
    from .colormnet_render import DEEPEX_SIZES
    if render_speed.lower() not in DEEPEX_SIZES:                                                  # get_deepex_size runs before the model switch: every ex_model
        raise HAVCError("HAVC_deepex: unknown render_speed ->" + render_speed)                     # deepex/__init__.py:50-83 (the same four names for ex_model 2)
    clip, single = _as_clip(clip)
    clip_ref, _ = _as_clip(clip_ref)
    n, h, w = clip.shape[:3]
    if clip_ref.shape[0] != n:
        raise HAVCError(f"HAVC_restore_video: clip_ref has {clip_ref.shape[0]} frames, clip has {n}")
    ref_thresh, ref_freq, ref_weight, merge = restore_video_params(method, ex_model, ref_merge, ref_weight, ref_thresh, ref_freq)
    # ---- everything below touches the GPU ----
    from . import scdetect
    device_index, debug = harness.get("device_index", 0), harness.get("debug")
    engine = dx = None
    if ex_model == 0:
        from .colormnet_render import DeepExColorMNet
        dx = DeepExColorMNet(vid_length=n, render_speed=render_speed, enable_resize=False, render_vivid=render_vivid, max_memory_frames=max_memory_frames,
                             frame_propagate=False, project_dir=torch_dir, state_dict=harness.get("state_dict"), device_index=device_index,
                             network=harness.get("network"))
        ctx = dx.ctx
    else:
        from .remaster_render import DEF_MIN_RF_FRAMES, RemasterClipRender, resize_for_inference_size
        memory_size = max(max_memory_frames or DEF_NUM_RF_FRAMES, DEF_MIN_RF_FRAMES)              # vsmodels.py:167-170
        engine = RemasterClipRender(device_index=device_index, ref_minedge=harness.get("ref_minedge", 256), ref_buffer_size=memory_size, length=2,
                                    state_dict=harness.get("state_dict"), model=harness.get("model"))
        ctx = engine._ctx()
    try:
        if tuple(clip_ref.shape[1:3]) != (h, w):
            clip_ref = spline36(ctx, clip_ref, w, h)                                               # :2057-2058
        coeffs = scdetect.LUMA_FULL if harness.get("luma_range", "limited") == "full" else scdetect.LUMA_LIMITED
        detected = scdetect.scene_detect(ctx, clip_ref, threshold=ref_thresh, frequency=ref_freq, frame_norm=ref_norm, coeffs=coeffs)
        if merge:
            scenes, clip_sc = scdetect.scene_detect(ctx, clip_ref, threshold=0, frequency=1, coeffs=coeffs), detected      # :2082-2083
        else:
            scenes, clip_sc = detected, None
        if debug is not None:
            debug.update(scenes=scenes, clip_sc=clip_sc, ref_weight=ref_weight, clip_ref=clip_ref)
        if ex_model == 0:
            return _colormnet_clip(dx, clip, clip_ref, scenes, clip_sc, ref_weight, single, None, debug)
        fw, fh = resize_for_inference_size(w, h, harness.get("frame_mindim", 320))
        host_in = not is_device(clip)
        dclip = DeviceImage.from_numpy(ctx, clip) if host_in else clip
        engine.load_clip_ref(clip_ref, (clip_sc if clip_sc is not None else scenes).scene_change_prev)       # remaster/__init__.py:109-112
        merge_weight = ref_weight if clip_sc is not None else 1.0                                  # :177
        small = spline64(ctx, dclip, fw, fh)
        colored = DeviceImage(ctx, small.shape)
        for n0 in range(0, n, 2):
            n1 = min(n0 + 2, n)
            colored.frames(n0, n1).copy_from(engine.process_clip_frames(small.frames(n0, n1), n0, min(n0 + 1, n - 1), merge_weight))
        out = spline64(ctx, colored, w, h, luma_from=dclip)
        out = F.chroma_post_process_np(ctx, out.as_rows(), dclip.as_rows()).reshaped(out.shape)    # vs_recover_clip_luma once more, :2125
        if host_in:
            out = out.numpy()
            return out[0] if single else out
        ctx.synchronize()
        return out.reshaped(out.shape[1:]) if single else out
    finally:
        if engine is not None:
            engine.close()
