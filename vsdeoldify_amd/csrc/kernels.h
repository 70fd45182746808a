// Internal launcher declarations shared by the HIP translation units of libhavc_mi355.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 half_t;

// a launch-constant divisor as multiplier + shift: n / d == fast_div(n, fd) for every 0 <= n < 2^31 (conv_common.h: fast_div_make, fast_div)
struct FastDiv { unsigned mul, sh; };

struct ConvArgs {
    const half_t* x;       // input NHWC fp16
    const half_t* w;       // packed weights [Npad][Kc][8] fp16
    const float* bias;     // [Npad] or null
    const float* scale;    // [Npad] or null (AFFINE)
    const float* shift;
    const half_t* res;     // residual NHWC fp16 or null
    void* y;               // output (fp16 NHWC / transposed fp16 / u8 RGB)
    int x_cpitch, x_coff;  // elements
    int res_cpitch, res_coff;
    int y_cpitch, y_coff;
    int Hi, Wi, C8;        // input spatial, number of 8-channel chunks
    int Ho, Wo, Co;        // output spatial, channels stored (multiple of 8; 3 for RGB8)
    int kh, kw, stride, pad, dil;
    int pad_w;             // pad along W (== pad except for ConvTranspose parity sub-convs)
    int oss, ooy, oox;     // output pixel = (ho*oss + ooy, wo*oss + oox) of an (Ho*oss) x (Wo*oss) image (oss 1 or 2)
    int Kc, Npad;          // weight matrix: Npad rows, Kc chunks (multiple of 4)
    int M;                 // batch*Ho*Wo
    int flags;
    int pix_pitch;         // transposed store: elements per channel row
    float f0, f1, f2;      // sigmoid range lo/hi, leaky slope
    float mean[3], istd[3];
    int cfg;               // 0 = heuristic; otherwise forced tile configuration (tools/conv_bench.py A/B runs)
    const int2* ktab;      // [Kc] per 16-byte K chunk: .x = byte offset of (tap, cin chunk) from the tap-0 pixel,
                           //      .y = dh | dw << 16 (input-pixel displacement of the tap; pad entries: dh = 0x7fff)
    int C8a;               // chunks of the main K segment (plan.py pack_conv); == C8 when there is no remainder segment
    int tiles_y, tiles_x;  // PS_BLUR / halo conv: 16x16-pixel GEMM-row tiles per frame (stride 15: one row / column of halo)
    const float* fuse_w;   // FUSE_RGB8: fp32 [3][Npad] weights of the fused 1x1 conv, fuse_b: its 3 biases
    const float* fuse_b;
    uint8_t* fuse_rgb;     // FUSE_RGB8: u8 RGB output [M][3]
    int cstore;            // PS_BLUR: channels actually stored per pixel (the packed rows may be padded to a multiple of 64); 0 = all
    float* fuse_out;       // FUSE_PROJ: fp32 output [M][Npad / 256][2]; fuse_w = fp32 [frame][2][256]
    unsigned x_bytes;      // size of the input allocation (buffer descriptor range; OOB lanes read zeros)
    unsigned w_bytes;      // Npad * Kc * 16
    int prio;              // 1: static s_setprio 1 for the younger half of an 8-wave block (HAVC_SETPRIO, default on)
    int splitk;            // > 1: the K range is cut into `splitk` parts, one block per (tile, part) stores its fp32 partial sums to `ws`
    float* ws;             //      [splitk][M][Npad]; splitk_reduce_kernel adds them in a fixed order and runs the usual epilogue
    float pscale;          // HAVC_F_PRECISE: the accumulator is this factor away from the convolution (2^-11 x the weight pre-scale, op.f3)
    int ngroup, rband;     // round 6, set by the pipelined launchers (conv_raster): > 0 = column tiles are walked in groups of `ngroup` inside bands of `rband` row tiles,
                           //      so that the weight panels one XCD has in flight fit its 4 MiB L2 (a 768 -> 3072 GEMM cycles 4.7 MB of weights per row tile otherwise)
    FastDiv fd_howo, fd_wo;    // the pixel index math of the kernels divides by Ho * Wo and Wo, the PS_BLUR kernels by tiles_y * tiles_x and tiles_x: filled with
    FastDiv fd_tt, fd_tx;      //      the rest of the struct (conv_set_divisors)
    int k_half_empty;          // 1: chunks 4..7 of the LAST stage of the K table are all pad entries -- the pipelined kernels skip that stage's second K half
};
// grouped tile order for GEMMs whose weight matrix does not fit an XCD's L2.  Same bytes: only the block -> tile map changes.  MEASURED AND LEFT OFF (round 6,
// profiles/r6_raster_group_ab.txt): on ConvNeXt-L's stage-2 pwconv1 (768 -> 3072, 128 frames) it cuts the kernel's HBM-side traffic from 2.13 to 1.76 GB per launch
// (fetch 1.33 -> 0.96 GB) but the launch gets 2 % SLOWER (0.728 -> 0.745 ms; c3 1 339 -> 1 338 frames/s): six weight panels plus the pixel tiles of the 32 blocks an XCD
// has in flight are still more than its 4 MiB, and every pixel tile is now read twice.  HAVC_RASTER_GROUP=1 switches it on (A/B).
inline void conv_raster(ConvArgs& a, int MT, int NT, int BN) {
    static const int on = [] { const char* e = getenv("HAVC_RASTER_GROUP"); return e ? atoi(e) : 0; }();
    a.ngroup = a.rband = 0;
    const double tile_bytes = (double)BN * a.Kc * 16.0;            // one column tile's weight panel
    if (!on || a.splitk > 1 || NT < 4 || MT < 16 || tile_bytes * NT < 3.5e6) return;
    int ng = (int)(2.5e6 / tile_bytes);
    if (ng < 2 || ng >= NT) return;                                  // (a panel of > 1.25 MB per column tile: nothing to group; huge-K layers stream their weights anyway)
    a.ngroup = ng;
    a.rband = (MT + 7) / 8;                                          // one band per XCD share of the row tiles
}
#define HAVC_KTAB_PAD_DH 0x7fff

// returns hipError_t as int
int launch_conv(const ConvArgs& a, hipStream_t s);
int launch_conv_pipe(const ConvArgs& a, int cfg, hipStream_t s);
int launch_conv_pipe_ef(const ConvArgs& a, int cfg, hipStream_t s);   // compile-time epilogue flags; -1 = no such kernel (conv_igemm_pipe_ef.hip)
bool conv_splitk_cfg_ok(int cfg);      // tile configurations that may run with ConvArgs::splitk > 1 (the plain pipelined tiles)
const char* conv_config_name(const ConvArgs& a);

int launch_maxpool3x3s2(const half_t* x, half_t* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cpitch,
                        int x_coff, int y_cpitch, int y_coff, hipStream_t s);
int launch_blur_resize(const half_t* x, half_t* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cpitch,
                       int x_coff, int y_cpitch, int y_coff, hipStream_t s);
int launch_affine(const half_t* x, half_t* y, const float* scale, const float* shift, int relu, int64_t npix, int C,
                  int x_cpitch, int x_coff, int y_cpitch, int y_coff, hipStream_t s);
int launch_copy_ch(const half_t* x, half_t* y, int64_t npix, int C, int x_cpitch, int x_coff, int y_cpitch,
                   int y_coff, hipStream_t s);
int launch_prep_rgb8(const uint8_t* rgb, half_t* y0, int y0_cpitch, int y0_coff, half_t* y1, int y1_cpitch,
                     int y1_coff, int64_t npix, hipStream_t s, int y1_fill = 0);   // y1_fill: pad channels behind y1's 8 that may be zeroed too
int launch_subsample2(const half_t* x, half_t* y, int B, int Ho, int Wo, int Hi, int Wi, int C, int x_cpitch, int x_coff,
                      int y_cpitch, int y_coff, hipStream_t s);
int launch_proj2(const half_t* x, int x_cpitch, int x_coff, int C, const float* w, const float* bias, int mode, float mul,
                 float* out, int64_t npix, hipStream_t s);
int launch_bilinear2(const float* x, float* y, int B, int Hi, int Wi, int Ho, int Wo, float mul, hipStream_t s);
int launch_prep_lab_l(const uint8_t* rgb, half_t* y, int y_cpitch, int y_coff, int64_t npix, hipStream_t s, int y_lo = 0);   // y_lo > 0: hi / lo pair (precise)
// Pillow 8bpc resample passes (integer coefficient tables from the host) and the Zhang post-process
int launch_pil_resize_passes(const uint8_t* src, int sw, int sh, uint8_t* tmp, uint8_t* dst, int dw, int dh, int n_frames,
                             const int* hb, const int* hk, int hks, const int* vb, const int* vk, int vks, hipStream_t s);
int launch_zhang_post(const uint8_t* orig, const float* ab, int abH, int abW, uint8_t* out, int n_frames, int w, int h,
                      hipStream_t s);
// attention: qk [B][N][qk_pitch] (f at f_coff, g at g_coff, d channels each), vT [B][dv][npitch],
// x/out NHWC; out = gamma*attn + x
int launch_attention(const half_t* qk, int qk_pitch, int f_coff, int g_coff, int d, const half_t* vT, int dv,
                     int npitch, const half_t* x, int x_cpitch, int x_coff, half_t* out, int o_cpitch, int o_coff,
                     int B, int N, float gamma, hipStream_t s);

// u8 colour filters (device pointers, interleaved RGB)
int launch_blend_u8(const uint8_t* a, const uint8_t* b, float w, uint8_t* out, int64_t nbytes, hipStream_t s);
int launch_yuv_merge(const uint8_t* color, const uint8_t* orig, uint8_t* out, int64_t npix, hipStream_t s);
int launch_chroma_stabilizer(const uint8_t* stable, const uint8_t* inew, double alpha, float weight, uint8_t* out,
                             int64_t npix, hipStream_t s);
int launch_luma_merge(const uint8_t* dark, const uint8_t* white, int mode, double tresh, double grad, uint8_t* out, int64_t npix,
                      hipStream_t s);
int launch_luma_sum(const uint8_t* img, unsigned long long* d_sum, int64_t npix, hipStream_t s);
int launch_chroma_temporal_limiter(const uint8_t* cur, const uint8_t* prv, double alpha, uint8_t* out, int64_t npix, hipStream_t s);
int launch_chroma_stabilizer_adaptive(const uint8_t* stable, const uint8_t* inew, float base_tol, float max_extra, float weight,
                                      uint8_t* out, int w, int h, hipStream_t s);
int launch_color_temporal_stabilizer(const uint8_t* const* frames, const double* weights, int n, uint8_t* out, int64_t npix,
                                     hipStream_t s);
// ddcolor.hip (+ the Lab wrapper kernels in zhang.hip)
int launch_prep_ddcolor(const uint8_t* rgb, half_t* y, int y_cpitch, int y_coff, half_t* y2, int y2_cpitch, int y2_coff, int64_t npix,
                        hipStream_t s, int precise = 0);
int launch_ddcolor_post(const uint8_t* orig, const half_t* ab, int ab_cpitch, int ab_coff, int abH, int abW, uint8_t* out_u8, void* out_planes,
                        int planes_half, int n_frames, int w, int h, hipStream_t s, int ab_lo = 0);          // ab_lo > 0: the ab map is a hi / lo pair tensor
int launch_planar_f_to_rgb8(const void* planes, int is_half, uint8_t* rgb, int64_t npix, hipStream_t s);
int launch_planar_to_rgb8(const uint8_t* planes, uint8_t* rgb, int64_t npix, hipStream_t s);
int launch_rgb8_to_planar(const uint8_t* rgb, uint8_t* planes, int64_t npix, hipStream_t s);
int launch_dwconv7(const half_t* x, const half_t* w, const float* bias, half_t* y, int B, int H, int W, int C, int x_cpitch, int x_coff,
                   int y_cpitch, int y_coff, int w_pitch, hipStream_t s);
bool dwconv7_ln_supported(int C);
int launch_dwconv7_ln(const half_t* x, const half_t* w, const float* bias, const float* gamma, const float* beta, float eps, half_t* y, int B,
                      int H, int W, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff, int w_pitch, hipStream_t s);
int launch_fold_queries(const half_t* e, int e_cpitch, int e_coff, int tok, const float* r, int r_pitch, int nq, float* out, int B, int C,
                        hipStream_t s);
int launch_shuf4_blur_ab(const float* proj, const half_t* img, int img_cpitch, int img_coff, const float* rimg, const float* bias, half_t* y,
                         int y_cpitch, int y_coff, int B, int Hi, int Wi, hipStream_t s);
int launch_shuf4_blur_ab_p(const float* proj, const half_t* img, int img_cpitch, int img_coff, const float* rimg, const float* bias, half_t* y,
                         int y_cpitch, int y_coff, int B, int Hi, int Wi, hipStream_t s);   // pair image, pair output (precise FUSE_PROJ tail)
int launch_layernorm_c(const half_t* x, half_t* y, const float* gamma, const float* beta, float eps, int64_t npix, int C, int x_cpitch,
                       int x_coff, int y_cpitch, int y_coff, hipStream_t s, int relu = 0);
int launch_mha32(const half_t* q, int q_cpitch, int q_coff, int q_tok, const half_t* kv, int kv_cpitch, int k_coff, int v_coff, int kv_tok,
                 half_t* o, int o_cpitch, int o_coff, int o_tok, int B, int heads, int Lq, int Lk, float scale, hipStream_t s);
int mha32_nsplit(int Lk);
int launch_mha32_split(const half_t* q, int q_cpitch, int q_coff, int q_tok, const half_t* kv, int kv_cpitch, int k_coff, int v_coff, int kv_tok,
                       half_t* o, int o_cpitch, int o_coff, int o_tok, float* part, int B, int heads, int Lq, int Lk, float scale, hipStream_t s);
int launch_pixshuf4_blur(const half_t* x, half_t* y, int B, int Hi, int Wi, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff,
                         hipStream_t s);
// tweaks.hip: image_tweak chain (Pillow hue shift, ImageEnhance Brightness / Contrast / Color, hue-range mask), Y table of
// luma_adjusted_levels, restore_color_gradient.
#define HAVC_MAX_HUE_RANGES 8
struct TweakArgs {
    int hue_offset;               // Pillow hue units (0..255 per turn); 0 = no hue shift
    float brightness, contrast, color;    // ImageEnhance factors; 1 = step skipped
    int mean_l;                   // Contrast: int(mean(L) + 0.5) of the image in front of the contrast step
    int n_ranges;                 // hue-range mask on the ORIGINAL image (degrees, strict inequalities); 0 = none
    double range_lo[HAVC_MAX_HUE_RANGES], range_hi[HAVC_MAX_HUE_RANGES];
};
int launch_image_tweak(const uint8_t* img, uint8_t* out, int64_t npix, const TweakArgs& a, unsigned long long* d_sum, bool sum_only,
                       hipStream_t s);
struct ChromaTweakArgs {
    int has_hue, has_adjust, has_hue2, has_sat2, n_ranges;
    double hue_half, satc, brightc, hue_half2, sat2c, weight;
    double range_lo[HAVC_MAX_HUE_RANGES], range_hi[HAVC_MAX_HUE_RANGES];
};
int launch_chroma_tweak(const uint8_t* img, uint8_t* out, int64_t npix, const ChromaTweakArgs& a, hipStream_t s);
int launch_luma_lut(const uint8_t* img, const uint8_t* d_lut, uint8_t* out, int64_t npix, hipStream_t s);
// stabilizer.hip: the HAVC_stabilizer filter chain (dark tweak -> chroma / bright tweak -> colormap) in ONE launch.  A stage = one of the two tweaks above
// followed by a luma-masked merge with the stage's input (the operands of launch_luma_merge; merge_mode -1: the tweaked pixel as it is).
#define HAVC_MAX_STAB_STAGES 3
struct StabStage {
    int kind;                     // 0 = image_tweak (tw), 1 = image_chroma_tweak (ct)
    int identity;                 // kind 1: the tweak hands its input on (np_image_chroma_tweak's early return); the merge still runs
    int merge_mode;               // -1 none, 0..3 = launch_luma_merge's modes
    double tresh, grad;
    TweakArgs tw;
    ChromaTweakArgs ct;
};
struct StabChainArgs { int n; StabStage st[HAVC_MAX_STAB_STAGES]; };
int launch_stabilizer_chain(const uint8_t* img, uint8_t* out, int64_t npix, const StabChainArgs& a, hipStream_t s);
// tiles.hip: HAVC_clip_slice / HAVC_clip_reconstruct (vsslib/vstiles4.py).  A clip [n][h][w][3] is cut into 2 (side by side) or 4 (2 x 2) overlapping tile
// clips [n][th][tw][3], tw = base_w + ox, th = base_h + oy (2 tiles: base_h = h, oy = 0), and blended back.  All pointers are device pointers.
struct TileArgs {
    uint8_t* tile[4];             // tl, tr, bl, br (2 tiles: tl, tr)
    int w, h, n;                  // size and frames of the clip
    int n_tiles;                  // 2 or 4
    int base_w, base_h, ox, oy;
    int mask_val;                 // reconstruct: 0 = linear ramp over the overlap, 1..255 = constant weight of the right / bottom tile
};
int launch_tile_slice(const uint8_t* clip, const TileArgs& a, hipStream_t s);
int launch_tile_reconstruct(const TileArgs& a, const uint8_t* orig, uint8_t* out, hipStream_t s);      // orig != null: luma of orig, chroma of the blend
// scdetect.hip: per-frame scene statistics of a clip [n][h][w][3] (gray sum, min, max, SAD against the frame `offset` frames before).  SceneRec is the
// layout of havc_scene_rec (include/havc_mi355.h); on the device min_y holds 255 - min until the runtime has downloaded the records.
struct SceneRec { long long sum_y, sad, sum_raw; int min_y, max_y; };
struct SceneStatsArgs {
    int n, h, w, offset;
    int cr, cg, cb, bias;         // Y = (cr * R + cg * G + cb * B + bias) >> 16, at most 255 (checked by havc_scene_stats)
    int normalize;                // frame_normalize between tht_black and tht_white: two dependent launches
    int blocks_per_frame;         // set by launch_scene_stats
    double tht_black, tht_white;
};
int launch_scene_stats(const uint8_t* clip, SceneRec* rec, SceneStatsArgs a, hipStream_t s);   // rec: n zero-filled device records
// scfilter.hip: the pixel work of the SSIM / histogram scene filter on a clip [n][h][w][3], frames named by index lists (device memory, checked by the
// caller).  out of launch_scene_hist: k zero-filled rows of 256 counters.  launch_scene_ssim: pairs = m x 2 frame numbers, partial = m *
// scene_ssim_tiles(h, w) doubles of workspace, out = m doubles; h, w >= 7.
constexpr int SCF_SSIM_TILE = 32;     // window positions per block and direction
int scene_ssim_tiles(int h, int w, int* tiles_x = nullptr, int* tiles_y = nullptr);
int launch_scene_hist(const uint8_t* clip, const int* idx, int k, unsigned* out, int h, int w, hipStream_t s);
int launch_scene_ssim(const uint8_t* clip, const int* pairs, int m, double* partial, double* out, int h, int w, hipStream_t s);
// scedge.hip: the edge-masked scene statistics of a clip [n][h][w][3] (vsslib/vsscdetect_edge.py:168-182).  EdgeRec is the layout of havc_edge_rec.
constexpr int EDGE_MAX_SIDE = 16384;  // width and height: keeps a wave's 32-bit partial sums exact (scedge.hip)
struct EdgeRec { long long sum_y, sad_prev, sad_next, sum_masked; };
struct EdgeStatsArgs {
    int n, h, w, offset;          // 1 <= offset < n
    int cr, cg, cb, bias;         // as SceneStatsArgs
    int radius;                   // 1..8: the blur's radius; wt[0 .. 2 radius] its weights, tap -radius first
    int blocks_per_frame, tiles_x, tiles_y;       // set by launch_scene_edge_stats
    float wt[17];
    uint8_t enh[256];             // the enhanced plane's table
};
int launch_scene_edge_stats(const uint8_t* clip, EdgeRec* rec, uint8_t* tap, EdgeStatsArgs a, hipStream_t s);   // rec: n zero-filled device records
// equalize.hip: rgb_equalizer methods 0-3 (CLAHE / equalizeHist) with rgb_balance in front, on a clip [n][h][w][3] (vsdeoldify/havc_utils.py:836-1145)
struct EqArgs {
    int n, h, w, method;          // method 0..3
    int luma_blend, range_tv, balance;
    int w15, w3_15, bal_w15;      // std.Merge weights as int(w * 32768 + 0.5): result <- input, method 0 <- method 1, balanced <- input
    double clip_limit;
    double factor[3];             // rgb_balance's rgb_factor
    uint8_t lut_in[256], lut_out[256];     // applied to every sample read / written
    int tile_w, tile_h, clip, blocks_per_frame;      // set by launch_equalize
    float lut_scale;
};
size_t equalize_workspace_bytes(int n, int method);
int launch_equalize(const uint8_t* src, uint8_t* dst, void* ws, EqArgs a, hipStream_t s);   // ws: see equalize.hip
int launch_restore_color_gradient(const uint8_t* color, const uint8_t* gray, uint8_t* out, int64_t npix, double sat, int tht, double alpha,
                                  double weight, int algo, int return_mask, hipStream_t s);
// recover.hip: HAVC_recover_clip_color / ChromaRetentionMerge on a clip [n][h][w][3] (vsslib/mcomb.py:450-516): per-frame luma sums, then the gated per-pixel
// restore (gradient mask: restore_color_gradient; binary mask: restore_color), two launches.  sums: n slots of device memory (zeroed by the launcher).
struct RecoverArgs {
    int n, h, w;
    int first_frame;              // clip index of frame 0: the binary path hands frames with index < 15 on unchanged
    double sat, weight, alpha;
    int tht, algo;                // algo 0..2 (gradient path)
    int binary_mask, return_mask;
    int luma_blocks, apply_blocks;   // blocks per frame of the two launches, set by launch_recover_color
};
int launch_recover_color(const uint8_t* gray, const uint8_t* color, uint8_t* out, unsigned long long* sums, RecoverArgs a, hipStream_t s);
// retinex.hip: HAVC_retinex = multi-scale Retinex (MSRCP) on a chunk of a clip [n][h][w][3] (vsslib/vsretinex.py:52-88; the plugin's pixel work restated from
// its published algorithm).  All of a chunk's frames and sigmas go through every launch together.
struct RetArgs {
    int n, h, w, ns;              // frames of the chunk, frame size, number of sigmas (1..8)
    int sF, sR, dF, dR;           // source / destination range: (0, 255) full, (16, 219) limited
    int range_tv, blend;
    double luma_dark, luma_bright;
    double coef[8][4];            // B, B1, B2, B3 per sigma (ret_coefficients)
    int blocks_per_frame;         // set by launch_retinex
};
size_t retinex_record_bytes(int n);                  // the per-frame records and histograms of n frames (zero-filled by the caller)
// planes: n * ns float64 planes of h * w; rec: retinex_record_bytes(n) bytes, zero-filled on the same stream in front of the call; tap_g / tap_p (both or
// neither, device memory): the n * ns Gaussian planes and the n MSR product planes, for the tests
int launch_retinex(const uint8_t* src, uint8_t* dst, double* planes, void* rec, double* tap_g, double* tap_p, RetArgs a, hipStream_t s);
// the channel sums of every frame alone (eq_chan_sum_kernel with an identity table): rec = n zero-filled EqFrameRec, only .chan is written
int launch_equalize_chan_sums(const uint8_t* src, void* rec, int n, int h, int w, hipStream_t s);
// tweak.hip: HAVC_tweak's RGB24 <-> YUV420P8 round trip (BT.709 full range, Mitchell bicubic chroma, error diffusion on the way back: the stand-in of
// tests/tweak_util.py) and HAVC_adjust_rgb as per-frame tables, on a clip [n][h][w][3] (vsslib/vsfilters.py:753-850, havc_utils.py:664-749)
#define TW_MAX_SIDE 4096          // width and height: the back kernel keeps one error row per channel in LDS
struct TweakWeights { float down_v[8], down_h[8], up_v[2][4], up_h[2][4]; };      // the chroma filters (tweak_ops.h: tw_all_weights), set by the launchers
struct TweakFwdArgs {
    int n, h, w;                  // frames of the chunk (at most 65535), frame size (even, at most TW_MAX_SIDE)
    int has_gamma, has_hue_sat, has_luma;
    float hue_c, hue_s;           // hue_cos * sat, hue_sin * sat as std.Expr's float32 constants
    uint8_t gamma_lut[256];       // applied to every RGB sample read
    uint8_t luma_lut[256];        // applied to every Y sample written
    TweakWeights wt;
};
struct TweakBackArgs { int n, h, w; TweakWeights wt; };
int launch_tweak_forward(const uint8_t* src, uint8_t* y, uint8_t* u, uint8_t* v, TweakFwdArgs a, hipStream_t s);
int launch_tweak_back(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* dst, TweakBackArgs a, hipStream_t s);
// the two variants havc_chroma_stab_clip needs (same kernel bodies): the back conversion with Y of frame yidx[f] and U, V of frame cidx[f] (device tables
// of a.n entries), and the forward conversion of restore_color(color frame color_idx[f], gray frame f) that keeps U and V only
struct TweakRestoreArgs {
    const uint8_t* color;                 // the clip the colours come from; frame color_idx[f] belongs to gray frame f
    const int* color_idx;
    const uint8_t* mode;                  // per frame: 0 = the gray frame as it is (clip frame < 15), 1 = restore_color with its gate
    const unsigned long long* stats;      // per frame: sum of cv2's Y, count of pixels with S < tht (launch_stab_stats)
    double sat, weight, tht_scen;
    int tht;
};
int launch_tweak_back_indexed(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* dst, const int* yidx, const int* cidx, TweakBackArgs a,
                              hipStream_t s);
int launch_tweak_forward_restore(const uint8_t* gray, uint8_t* u, uint8_t* v, TweakFwdArgs a, TweakRestoreArgs ra, hipStream_t s);
// vformat.hip: a clip's own planes (YUV 4:2:0 / 4:2:2 / 4:4:4 or GRAY, 8..16 bit, limited or full range, four matrices) <-> RGB24: the stand-in of
// tests/vformat_util.py, built on the resampler, the mirroring and the error diffusion above.  The launchers derive every constant from these fields.
struct VfArgs {
    int n, h, w;                  // frames of the chunk, frame size (at most TW_MAX_SIDE; even where the chroma is subsampled)
    int gray, sub_w, sub_h;       // GRAY: one plane; log2 chroma subsampling (1, 1), (1, 0) or (0, 0)
    int bits;                     // 8: uint8 planes; 9..16: uint16 planes
    int matrix;                   // 1, 5, 6, 9 (H.273)
    int full_range;               // range of the matrix step
    int depth_full_range;         // planes -> RGB24: range of the > 8 bit -> 8 bit step in front of it
    int dither;                   // 0 round half to even, 1 error diffusion
    // set by the launchers (vf_constants)
    float kr, kg, kb, cb_div, cr_div, r_cr, b_cb, g_cr, g_cb;
    float y_off, y_scale, c_scale;        // planes -> RGB24 on 8-bit codes: Y = (y - y_off) / y_scale, C = (c - 128) / c_scale
    float depth_mul, depth_half;          // the depth step: limited v 2^-(bits - 8); full v (255 / (2^bits - 1)), chroma (v - 2^(bits - 1)) (..) + 128
    float ys, yo, cs, co, hi;             // RGB24 -> planes: Y ys + yo, C cs + co, codes clamped to [0, hi]
    TweakWeights wt;
};
int launch_vformat_to_rgb(const void* y, const void* u, const void* v, uint8_t* dst, VfArgs a, hipStream_t s);
int launch_vformat_from_rgb(const uint8_t* src, void* y, void* u, void* v, VfArgs a, hipStream_t s);
// chroma_stab.hip: what HAVC_stabilizer(stab=True) adds around those -- the index tables of a chunk, the per-frame sums of the shifted clips,
// std.AverageFrames on the U / V planes, ReduceFlicker (vsslib/vsfilters.py:38-63, 84-157, 216-356; the stand-ins of tests/stab_util.py)
struct StabTableArgs {
    int S, s0;                            // frames the chunk stabilises: clip frames s0 .. s0 + S - 1
    int A, a0;                            // source frames of the chunk: a0 .. a0 + A - 1 (at most 1024)
    int last, first_frame;                // last frame of the clip; clip index of frame 0 (the n < 15 rule)
    int N, restore;                       // weights; restore != 0: tht > 0 (list form over restored clips), 0: temporal form with the scene walk
    uint32_t prev_bits[32], next_bits[32];   // bit i: source frame a0 + i carries _SceneChangePrev / _SceneChangeNext
};
// pair_y / pair_c / pair_mode: S * (N - 1) entries (restore != 0); avg_tab: S * N plane numbers of the U / V pools
int launch_stab_tables(StabTableArgs a, int* pair_y, int* pair_c, uint8_t* pair_mode, int* avg_tab, hipStream_t s);
// stats: 2 * n zero-filled slots; frames with mode[f] == 0 are skipped
int launch_stab_stats(const uint8_t* gray, const uint8_t* mode, unsigned long long* stats, int n, int h, int w, int tht, hipStream_t s);
struct StabAverageArgs { int S, N, weights[15]; int64_t plane_bytes; };
int launch_stab_average(const uint8_t* upool, const uint8_t* vpool, uint8_t* uo, uint8_t* vo, const int* avg_tab, StabAverageArgs a, hipStream_t s);
// frames: clip frames t0 .. of the stabilised clip (every frame n - 2 .. n + 2 of an interior output frame is among them); out: frames f0 .. f0 + count - 1
int launch_reduce_flicker(const uint8_t* frames, int t0, uint8_t* out, int f0, int count, int last, int64_t frame_bytes, hipStream_t s);
struct AdjustArgs {
    int n, h, w;
    int mode;                     // 0: no normalisation, 1: vs_rgb_normalize, 2: std.Merge(clip, normalised, strength)
    int w15;                      // mode 2: int(strength * 32768 + 0.5)
    float gain[3], bias[3];       // "x r * rb +"
    uint8_t gamma_lut[3][256];    // std.Levels(gamma=) per plane (identity: none)
    int blocks_per_frame;         // set by launch_adjust_rgb
};
// rec: n zero-filled EqFrameRec (used with mode != 0); tables: n * 768 bytes; both device memory
int launch_adjust_rgb(const uint8_t* src, uint8_t* dst, void* rec, uint8_t* tables, AdjustArgs a, hipStream_t s);
// lut3d.hip: HAVC_TimeCube's 3D LUT on a clip, trilinear (the stand-in of tests/timecube_util.py).  table: [size^3][3] floats, red fastest; points: room for
// size^3 * 16 bytes (the padded copy the first launch writes); idx / frac: the axis tables [3][256]; all device memory.  Two launches.
struct Lut3dArgs { int64_t npix; int size; };     // pixels of the whole clip; lattice points per axis (2..256)
int launch_lut3d(const uint8_t* src, uint8_t* dst, const float* table, void* points, const int* idx, const float* frac, Lut3dArgs a, hipStream_t s);
// overlay.hip: HAVC_clip_overlay on RGB24 clips (the stand-in of tests/overlay_util.py), one launch
struct OverlayArgs {
    int n, bw, bh, ow, oh;        // frames; base and overlay size
    int x, y;                     // where the overlay's top left corner lies on the base (either sign)
    int mode, plane_mask;         // OverlayMode (overlay_ops.h); bit k: plane k is processed
    int mask_planes, first_plane; // 0: no mask, 1: [oh][ow], 3: [oh][ow][3]; first_plane != 0: plane 0 of a 3-plane mask serves every plane
    int overlay_frames;           // 1 (repeated) or n; the mask has as many
    float opacity;
};
int launch_overlay(const uint8_t* base, const uint8_t* ov, const uint8_t* mask, uint8_t* dst, OverlayArgs a, hipStream_t s);
// metrics.hip: per-pixel CIEDE2000 between two RGB24 clips in float64 (metrics_ops.h has the arithmetic, the restatement of oracle/imaging.py).  DeRec is the
// device image of havc_de_rec (include/havc_mi355.h); `max` travels as the bit pattern of a non-negative double, which orders like the value.
#define DE_BINS 1025
#define DE_BLOCK_PIXELS 1024          // 256 threads x 4 pixels: one partial sum per block
struct DeRec { double sum; unsigned long long max_bits; unsigned long long sse[3]; unsigned hist[DE_BINS]; unsigned reserved; };
inline int64_t delta_e_blocks(int64_t npix) { return (npix + DE_BLOCK_PIXELS - 1) / DE_BLOCK_PIXELS; }       // per frame
// a, b: [n][npix][3]; lin: the 256-entry sRGB -> linear table; rec: n zero-filled records; partials: n * delta_e_blocks(npix) doubles; map: NULL or [n][npix].
// n <= 65535 (grid y), npix <= 2^30.  Two launches: the pixels, then the per-frame sums in block order.
int launch_delta_e(const uint8_t* a, const uint8_t* b, const double* lin, DeRec* rec, double* partials, double* map, int n, int64_t npix, hipStream_t s);
// separable polyphase resample of interleaved u8 RGB (tap tables from the host; Spline64 = harness stand-in
// for zimg resize.Spline64).  orig != null fuses chroma_post_process (luma of orig, chroma of the resampled).
int launch_resize_passes(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, int n_frames, float* tmp,
                         const int* h_start, const float* h_w, int h_taps, const int* v_start, const float* v_w,
                         int v_taps, const uint8_t* orig, hipStream_t s);
// the horizontal kernel launch_resize_passes picks for a shape (host arithmetic only): 0 = resize_h_kernel, else the TMAX of resize_h_rows_kernel<TMAX>;
// *span_lds (optional) = the LDS bytes reserved for a 256-column tile's source span
constexpr int RESIZE_H_ROWS_PER_BLOCK = 16;
int resize_h_variant(int sw, int dw, int h_taps, int64_t rows, int* span_lds = nullptr);

// ---- ColorMNet memory kernels (colormnet.hip) ----
int launch_mem_similarity(const float* mk, const float* ms, const float* qk, const float* qe, float* sim, int B, int CK, int N, int HW, hipStream_t s,
                          int64_t mpitch = 0);      // mpitch / vpitch: row pitch of mk / mv in elements (0 = N: the reference's contiguous tensors)
int launch_mem_usage(const int* idx, const float* wgt, unsigned long long* acc, float* usage, int B, int N, int HW, int K, hipStream_t s);
int launch_mem_dense_readout(const float* sim, const float* mv, float* out, int B, int CV, int N, int P, hipStream_t s);
int mem_topk_splits(int N);
int launch_mem_similarity_t(const float* mk, const float* ms, const float* qk, const float* qe, float* simT, int B, int CK, int N, int HW, hipStream_t s,
                            int64_t mpitch = 0);
bool mem_topk_select_supported(int N);
int launch_mem_topk_select_readout(const float* simT, const float* mv, int* idx, float* wgt, float* out, int B, int CV, int N, int HW, int K, hipStream_t s,
                                   int64_t vpitch = 0);
int launch_mem_topk_readout(const float* sim, const float* mv, int* idx, float* wgt, float* cand_val, int* cand_idx, float* out, int B, int CV, int N,
                            int HW, int K, hipStream_t s, int64_t vpitch = 0);
int launch_mem_usage_update(const int* idx, const float* wgt, unsigned long long* acc, float* use, float* life, int from, int N, int HW, int K, hipStream_t s);
int launch_cmn_value_in(const float* img, const float* planes, float* vin, int64_t P, hipStream_t s);
int launch_vec_add(float* y, const float* x, int64_t n, hipStream_t s);
int launch_cmn_frame_in(const uint8_t* rgb, float* lab, float* img, int w, int h, int Wp, int Hp, int pad_l, int pad_t, hipStream_t s);
int launch_cmn_frame_out(const float* l_plane, const float* ab, uint8_t* rgb, int w, int h, int Wp, int Hp, int pad_l, int pad_t, hipStream_t s);
int launch_local_correlation(const float* q, const float* k, float* out, int n, int C, int H, int W, int R, int dil, float qscale, hipStream_t s);
int launch_local_softmax(float* qk, const float* q, const float* rel_w, const float* rel_b, int n, int C, int H, int W, int R, int dil, hipStream_t s);
int launch_local_agg(const float* attn, const float* v, float* agg, int n, int CV, int H, int W, int R, int dil, hipStream_t s);

int launch_range_stats(const void* p, int elem_bytes, int64_t n, unsigned* stats, hipStream_t s);

// ---- eager module load + big-LDS opt-ins, one function per translation unit (called once per device from havc_create) ----
void preload_conv_pipe();
void preload_conv_pipe_ef();
void preload_conv_igemm();
void preload_elementwise();
void preload_zhang();
void preload_attention();
void preload_colorfilters();
void preload_tweaks();
void preload_stabilizer();
void preload_tiles();
void preload_recover();
void preload_scdetect();
void preload_scfilter();
void preload_scedge();
void preload_equalize();
void preload_retinex();
void preload_tweak_clip();
void preload_chroma_stab();
void preload_lut3d();
void preload_overlay();
void preload_metrics();
void preload_ddcolor();
void preload_colormnet();
void preload_colormnet_net();
void preload_precise();
void preload_remaster();

// ---- precise mode (precise.hip): the non-conv ops of the DeOldify generators on hi / lo fp16 pairs, fp32 arithmetic ----
int launch_prep_rgb8_p(const uint8_t* rgb, half_t* y0, int y0_cpitch, int y0_coff, half_t* y1, int y1_cpitch, int y1_coff, int64_t npix, hipStream_t s);
int launch_maxpool3x3s2_p(const half_t* x, half_t* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff,
                          hipStream_t s);
int launch_blur_resize_p(const half_t* x, half_t* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff,
                         hipStream_t s);
int launch_affine_p(const half_t* x, half_t* y, const float* scale, const float* shift, int relu, int64_t npix, int C, int x_cpitch, int x_coff, int y_cpitch,
                    int y_coff, hipStream_t s);
bool attention_p_supported(int d, int C);
bool attention_pm_supported(int d, int C, int npitch);
int launch_attention_pm(const half_t* qk, int qk_cpitch, int f_coff, int g_coff, int d, int64_t qk_fs, const half_t* vT, int npitch, int64_t v_fs,
                        const half_t* x, int x_cpitch, int x_coff, int64_t x_fs, half_t* out, int o_cpitch, int o_coff, int64_t o_fs, float* stats, int B, int N,
                        int C, float gamma, hipStream_t s);
// precise2.hip: the non-conv ops of DDColor and the Zhang colorizers on hi / lo pairs
int launch_proj2_p(const half_t* x, int x_cpitch, int x_coff, int C, const float* w, const float* bias, int mode, float mul, float* out, int64_t npix,
                   hipStream_t s);
int launch_layernorm_p(const half_t* x, half_t* y, const float* gamma, const float* beta, float eps, int64_t npix, int C, int x_cpitch, int x_coff,
                       int y_cpitch, int y_coff, int relu, hipStream_t s);
bool dwconv7_ln_p_supported(int C);      // precise fused dwconv 7x7 + LayerNorm (ddcolor.hip): 192 / 384 / 768 channels
int launch_dwconv7_ln_p(const half_t* x, const float* w, const float* bias, const float* gamma, const float* beta, float eps, half_t* y, int B,
                        int H, int W, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff, int w_pitch, hipStream_t s);
int launch_dwconv7_p(const half_t* x, const float* w, const float* bias, half_t* y, int B, int H, int W, int C, int x_cpitch, int x_coff, int y_cpitch,
                     int y_coff, int w_pitch, hipStream_t s);
int launch_mha32_p(const half_t* q, int q_cpitch, int q_coff, int q_tok, const half_t* kv, int kv_cpitch, int k_coff, int v_coff, int kv_tok, half_t* o,
                   int o_cpitch, int o_coff, int o_tok, int B, int heads, int Lq, int Lk, float scale, hipStream_t s);
int launch_fold_queries_p(const half_t* e, int e_cpitch, int e_coff, int tok, const float* r, int r_pitch, int nq, float* out, int B, int C, hipStream_t s);
int launch_shuf4_blur_proj_p(const half_t* x, int x_cpitch, int x_coff, const float* M, const half_t* img, int img_cpitch, int img_coff, const float* rimg,
                             const float* bias, half_t* y, int y_cpitch, int y_coff, int B, int Hi, int Wi, hipStream_t s);
int launch_subsample2_p(const half_t* x, half_t* y, int B, int Ho, int Wo, int Hi, int Wi, int C, int x_cpitch, int x_coff, int y_cpitch, int y_coff,
                        hipStream_t s);
void preload_precise2();
int launch_attention_p(const half_t* qk, int qk_cpitch, int f_coff, int g_coff, int d, int64_t qk_fs, const half_t* h, int h_cpitch, int h_coff, int64_t h_fs,
                       const half_t* x, int x_cpitch, int x_coff, int64_t x_fs, half_t* out, int o_cpitch, int o_coff, int64_t o_fs, float* stats, int B, int N,
                       int C, float gamma, hipStream_t s);

// ---- ColorMNet network kernels (colormnet_net.hip) ----
#ifndef HAVC_EW_SRC_BCAST          // (public values: include/havc_mi355.h)
#define HAVC_EW_SRC_BCAST 1
#define HAVC_EW_RES 2
#define HAVC_EW_RES_BCAST 4
#define HAVC_EW_RELU 8
#define HAVC_EW_DUAL 16
#endif
struct EwArgs {
    const half_t* x; half_t* y; const half_t* res; half_t* y2;
    int B, Hi, Wi, Ho, Wo, C8;
    int x_cp, x_co, y_cp, y_co, r_cp, r_co, y2_cp, y2_co;
    int64_t x_fs, y_fs, r_fs, y2_fs;          // frame strides in elements (0 = the same frame for every batch entry)
    int mode, factor, flags;                  // mode 0 copy, 1 bilinear (align_corners = False), 2 area (factor x factor mean)
    float rh, rw;                             // bilinear source / destination ratios
};
int launch_ew(const EwArgs& a, hipStream_t s);
int launch_dwconv(const half_t* x, const half_t* w, const float* bias, half_t* y, int B, int H, int W, int C, int K, int x_cp, int x_co, int64_t x_fs,
                  int y_cp, int y_co, int64_t y_fs, int w_pitch, hipStream_t s);
int chan_attn_splits(int P, int heads, int c);
int launch_chan_attn(const half_t* q, int q_cp, int q_co, int64_t q_fs, const half_t* k, int k_cp, int k_co, int64_t k_fs, const float* temp,
                     float* part_g, float* part_n, half_t* wout, int64_t w_fs, int w_pitch, int B, int P, int heads, int c, hipStream_t s);
int launch_mha64(const half_t* qkv, int cp, int q_co, int k_co, int v_co, int tok, half_t* o, int o_cp, int o_co, int o_tok, int B, int heads, int L,
                 float scale, hipStream_t s);
int launch_cbam(const half_t* x, int cp, int co, int64_t fs, int B, int H, int W, int C, const float* w1, const float* b1, const float* w2, const float* b2,
                const float* w7, const float* b7, float* scale, float* comp, half_t* y, int y_cp, int y_co, int64_t y_fs, half_t* y2, int y2_cp, int y2_co,
                int64_t y2_fs, hipStream_t s);
int launch_gru(const half_t* v, int cp, int co, int64_t fs, const float* h, float* out, int B, int P, int hd, hipStream_t s);
int launch_cmn_decoder_in(const half_t* g, int g_cp, int g_co, const float* ro, int64_t ro_fs, const float* hid, int64_t hid_fs, half_t* y, half_t* y2, int cp,
                          int co, int64_t fs, int B, int P, int Cg, int CV, int HD, hipStream_t s);
int launch_planar_in(const float* x, int64_t x_fs, half_t* y, int cp, int co, int64_t fs, int B, int P, int C, int span, int pixel_major, int bcast,
                     hipStream_t s);
int launch_planar_out(const half_t* x, int cp, int co, int64_t fs, float* y, int64_t y_fs, int B, int P, int C, int act, hipStream_t s);
// the frame wrapper of ColorMNetRender (zhang.hip: skimage Lab formulas in fp64)
int launch_cmn_rgb_to_lab(const uint8_t* rgb, float* lab, int64_t npix, hipStream_t s);
int launch_cmn_lab_to_rgb(const float* l_plane, const float* ab, uint8_t* rgb, int64_t npix, hipStream_t s);

// ---- DeepRemaster colour network (remaster.hip) ----
bool srcref_attention_supported(int d, int dv);
// q: [T][nq_frame][q_pitch] (64 channels at q_coff), k: [Tr][nk_frame][64], vT: [Tr][512][npitch]; x / out: the source and result views, T frames
int launch_srcref_attention(const half_t* q, int q_pitch, int q_coff, int64_t q_fs, const half_t* k, int64_t k_fs, const half_t* vT, int npitch, int64_t v_fs,
                            const half_t* x, int x_pitch, int x_coff, int64_t x_fs, half_t* out, int o_pitch, int o_coff, int64_t o_fs, int T, int nq_frame,
                            int Tr, int nk_frame, float gamma, hipStream_t s);
int launch_tstack(const half_t* x, half_t* y, int T, int64_t P, int C, int x_cp, int x_co, int64_t x_fs, int y_cp, int y_co, int64_t y_fs, hipStream_t s);
int launch_elu(const half_t* x, half_t* y, int B, int64_t P, int C, int x_cp, int x_co, int64_t x_fs, int y_cp, int y_co, int64_t y_fs, hipStream_t s);
int launch_prep_remaster(const uint8_t* rgb, half_t* y, int B, int Hi, int Wi, int Ho, int Wo, int refs, int y_cp, int y_co, int64_t y_fs, hipStream_t s);
int launch_remaster_out(const half_t* ab, int ab_cp, int ab_co, int64_t ab_fs, const uint8_t* rgb_in, uint8_t* out, float* ab_out, int B, int64_t P, hipStream_t s);
