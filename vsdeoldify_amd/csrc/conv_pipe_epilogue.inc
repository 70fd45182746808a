// The shared epilogue of conv_pipe_kernel and conv_halo_kernel -- TEXTUALLY INCLUDED inside the kernel bodies (conv_igemm_pipe.hip).
// PF(mi): the pixel fragment (0..FM-1) accumulator index mi belongs to (identity unless the EXTRA tile rotates its waves' fragment order).
// Expects in scope: p, acc[FN][FM], accx[2], smem, tid, lane, wave, wm, wn, lr, lg, m0, n0, has_extra, HoWo, the constants
// WM WN FM EXTRA ABL NW BM BN, lp = the pixel (0..15) of the 16-pixel fragment that MFMA column lr carries, and eflags (the op's flags: p.flags, or with the epilogue bits fixed at compile time), gm(local_row) -> GEMM row "m" of tile row local_row (>= p.M when the row is outside the
// problem; opix(m) is then the output pixel: out_pixel(p, m, HoWo), or m itself where the out step is known to be 1).
    // ---- epilogue ----
    if (ABL == 5 || ABL == 9 || ABL == 10) {
        float t = 0.f;
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) t += acc[ni][mi][0] + acc[ni][mi][1] + acc[ni][mi][2] + acc[ni][mi][3];
        if (t == 123.456f) reinterpret_cast<half_t*>(p.y)[0] = (half_t)t;
        return;
    }
    // Main 256 columns: transpose through LDS so every lane stores 16 B and 8 lanes cover one 128-byte line of a pixel
    // (the direct fragment layout gives 8-byte stores in 32-byte runs: 0.29 ms of a 1.6 ms launch, fully exposed at one
    // block per CU).  Phase 1: bias -> ReLU -> affine in registers, fp16, ds_write_b64 into a wave-private
    // [8 fragments][16 pixels][128 B] image (16-byte slots XOR-swizzled by pixel).  Phase 2: ds_read_b128, residual +
    // ReLU, global store.  TRANSPOSED / RGB8 / odd pixel-shuffle widths keep the per-fragment path.
    constexpr bool PRECISE = (ABL == 30);                  // precise mode: per-fragment fp32 epilogue storing hi / lo pairs (conv_common.h)
    const bool lds_epi = !PRECISE && !(eflags & (HAVC_F_OUT_TRANSPOSED | HAVC_F_OUT_RGB8)) &&
                         (!(eflags & HAVC_F_OUT_PIXSHUF) || (p.Co & 63) == 0);
    bool fused_done = false;
    if (PRECISE && EXTRA && has_extra && (eflags & HAVC_F_FUSE_RGB8)) {
        // ---- precise form of HAVC_F_FUSE_RGB8 (round 5): layers.11 (1x1 conv -> 3 channels) + SigmoidRange + denormalise + trunc u8 in fp32 ----
        // r2 = ReLU(acc * pscale + bias) + residual stays in registers as fp32 (no fp16 rounding point anywhere); every lane folds its 4 channels of
        // every fragment into three partial dot products per pixel, the four lane groups of a pixel are added by shuffles, the four N-waves and the
        // extra-column fragment through LDS in a FIXED order.  Saves the r2 pair tensor (5.3 GB written + read per 16 frames at 560 x 560) and a launch.
        fused_done = true;
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int rlo = p.res_cpitch >> 1;
        auto fold = [&](const float4v a4, int m, int n, float d[3]) {
            if (n >= p.Npad) return;
            float v[4];
            const float4 bv = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = a4[r] * p.pscale + bb[r];
                if (eflags & HAVC_F_RELU_PRE) v[r] = v[r] > 0.f ? v[r] : (leaky ? v[r] * p.f2 : 0.f);
            }
            if ((eflags & HAVC_F_RESIDUAL) && m < p.M && n < p.Co) {
                const half_t* rp = p.res + opix(m) * p.res_cpitch + p.res_coff + n;
                const half4 rh = *reinterpret_cast<const half4*>(rp), rl = *reinterpret_cast<const half4*>(rp + rlo);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += join_hl(rh[r], rl[r]);
            }
#pragma unroll
            for (int jo = 0; jo < 3; ++jo) {
                const float4 w4 = *reinterpret_cast<const float4*>(p.fuse_w + jo * p.Npad + n);
                d[jo] += v[0] * w4.x + v[1] * w4.y + v[2] * w4.z + v[3] * w4.w;
            }
        };
        float dsum[FM][3], dx[2][3];
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
            const int m = gm(wm * (FM * 16) + PF(mi) * 16 + lp);
            dsum[mi][0] = dsum[mi][1] = dsum[mi][2] = 0.f;
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) fold(acc[ni][mi], m, n0 + wn * 64 + ni * 16 + lg * 4, dsum[mi]);
#pragma unroll
            for (int jo = 0; jo < 3; ++jo) { dsum[mi][jo] += __shfl_xor(dsum[mi][jo], 16); dsum[mi][jo] += __shfl_xor(dsum[mi][jo], 32); }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = gm(wm * (FM * 16) + (wn * 2 + i) * 16 + lp);
            dx[i][0] = dx[i][1] = dx[i][2] = 0.f;
            fold(accx[i], m, n0 + BN + lg * 4, dx[i]);
#pragma unroll
            for (int jo = 0; jo < 3; ++jo) { dx[i][jo] += __shfl_xor(dx[i][jo], 16); dx[i][jo] += __shfl_xor(dx[i][jo], 32); }
        }
        __syncthreads();                                   // every wave is done reading the last stage
        float* part = reinterpret_cast<float*>(smem);      // [5][BM][3]
        if (lg == 0) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                float* q = part + (wn * BM + wm * (FM * 16) + PF(mi) * 16 + lp) * 3;
                q[0] = dsum[mi][0]; q[1] = dsum[mi][1]; q[2] = dsum[mi][2];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float* q = part + (4 * BM + wm * (FM * 16) + (wn * 2 + i) * 16 + lp) * 3;
                q[0] = dx[i][0]; q[1] = dx[i][1]; q[2] = dx[i][2];
            }
        }
        __syncthreads();
        for (int pl = threadIdx.x; pl < BM; pl += NW * 64) {
            const int m = gm(pl);
            if (m >= p.M) continue;
            uint8_t* y = p.fuse_rgb + opix(m) * 3;
#pragma unroll
            for (int jo = 0; jo < 3; ++jo) {
                float t = p.fuse_b[jo];
#pragma unroll
                for (int w = 0; w < 5; ++w) t += part[(w * BM + pl) * 3 + jo];
                float sg = 1.f / (1.f + expf(-t));
                sg = sg * (p.f1 - p.f0) + p.f0;
                sg = sg * p.istd[jo] + p.mean[jo];
                sg = fminf(fmaxf(sg, 0.f), 1.f);
                y[jo] = (uint8_t)(int)(sg * 255.f);
            }
        }
    } else if (PRECISE && !EXTRA && (eflags & HAVC_F_FUSE_PROJ) && WM == 2 && WN == 4 && FM == 8) {
        // ---- precise form of HAVC_F_FUSE_PROJ (round 6; DDColor: einsum + refine folded into a per-frame 2 x 256 projection, applied to every 256-column
        // tile of the last_shuf conv) ----  v = acc * pscale + bias, ReLU stays in registers as fp32; every lane folds its 16 channels into the two partial dot
        // products of its pixel (fp32 FMAs in a fixed order), the four lane groups of a pixel are added by shuffles, the four N-waves through LDS in a FIXED
        // order.  The 4096-channel pair tensor (4.3 GB per 16 frames at 128 x 128) is never written or re-read; shuf4_blur_ab_kernel<PREC> shuffles + blurs the
        // resulting fp32 2-channel map.  (The unfused precise chain rounded the conv output to a pair before the projection; this keeps it in fp32.)
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int nw0 = n0 + wn * 64, cw0 = wn * 64;
        float4 bvs[FN], w0[FN], w1[FN];
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
            bvs[ni] = p.bias ? *reinterpret_cast<const float4*>(p.bias + nw0 + ni * 16 + lg * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        float dsum[FM][2];
        int fb_prev = -1;
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
            const int mf = gm(wm * (FM * 16) + mi * 16);    // a 16-pixel fragment lies in one frame (Ho * Wo % 16 == 0)
            const int fb = mf < p.M ? mf / HoWo : 0;
            if (fb != fb_prev) {
                fb_prev = fb;
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) {
                    w0[ni] = *reinterpret_cast<const float4*>(p.fuse_w + ((size_t)fb * 2 + 0) * 256 + cw0 + ni * 16 + lg * 4);
                    w1[ni] = *reinterpret_cast<const float4*>(p.fuse_w + ((size_t)fb * 2 + 1) * 256 + cw0 + ni * 16 + lg * 4);
                }
            }
            float d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) {
                const float bb[4] = {bvs[ni].x, bvs[ni].y, bvs[ni].z, bvs[ni].w};
                const float a0[4] = {w0[ni].x, w0[ni].y, w0[ni].z, w0[ni].w}, a1[4] = {w1[ni].x, w1[ni].y, w1[ni].z, w1[ni].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[ni][mi][r] * p.pscale;
                    v += bb[r];
                    if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                    d0 = fmaf(v, a0[r], d0);
                    d1 = fmaf(v, a1[r], d1);
                }
            }
            d0 += __shfl_xor(d0, 16); d0 += __shfl_xor(d0, 32);
            d1 += __shfl_xor(d1, 16); d1 += __shfl_xor(d1, 32);
            dsum[mi][0] = d0; dsum[mi][1] = d1;
        }
        __syncthreads();                                   // every wave is done reading the last stage
        float* part = reinterpret_cast<float*>(smem);      // [4][BM][2]
        if (lg == 0) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                float* q = part + (wn * BM + wm * (FM * 16) + mi * 16 + lp) * 2;
                q[0] = dsum[mi][0]; q[1] = dsum[mi][1];
            }
        }
        __syncthreads();
        const int NTp = p.Npad >> 8, jt = n0 >> 8;
        for (int pl = threadIdx.x; pl < BM; pl += NW * 64) {
            const int m = gm(pl);
            if (m >= p.M) continue;
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { t0 += part[(w * BM + pl) * 2]; t1 += part[(w * BM + pl) * 2 + 1]; }
            *reinterpret_cast<float2*>(p.fuse_out + ((size_t)m * NTp + jt) * 2) = make_float2(t0, t1);
        }
        return;
    } else if (PRECISE && !EXTRA && (eflags & HAVC_F_PS_BLUR) && WM == 2 && WN == 4 && FM == 8) {
        // ---- precise form of HAVC_F_PS_BLUR (round 6): PixelShuffle(2) + ReplicationPad(1,0,1,0) + AvgPool2d(2,1) on hi / lo pairs out of LDS ----
        // (CustomPixelShuffle_ICNR, vsdeoldify/deoldify/unet.py:24-52; the reference runs it in fp32.)  The unfused precise chain stores the shuffled conv
        // result as a pair tensor (2 x the fp16 tensor: 5.1 GB per 16 frames at 560 x 560), reads it back in blur_resize_p and writes the blurred pairs:
        // here the shuffled values never leave the CU.  Same arithmetic, same rounding points -- v = acc * pscale + bias, ReLU, ROUNDED TO ITS PAIR
        // (join(split(v)): what the unfused conv stores), window sum ((TL + TR) + BL) + BR in fp32, x 0.25, split -- so the bytes are those of
        // the two-op chain (tests/test_gpu_precise.py).  A pair image of the whole 256 x 256 tile is 256 KiB; the tile goes through the 128 KiB of LDS in
        // TWO passes of 32 channels per sub-pixel: per (tile row, pixel) 128 B = [4 hi chunks | 4 lo chunks] of 8 channels, 16-byte slots XOR-swizzled by
        // pixel as in the fp16 form.  wave (wm, q) owns rows wm*8..+7 of sub-pixel q; 480 threads = 30 output rows x 4 column segments x 4 chunks.
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int nw0 = n0 + wn * 64;
        float4 bvA[FN];
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) bvA[ni] = p.bias ? *reinterpret_cast<const float4*>(p.bias + nw0 + ni * 16 + lg * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        char* img = smem + wave * (FM * 2048);
        const int tile = m0 / BM, tt = p.tiles_y * p.tiles_x;
        const int b = tile / tt, t = tile - b * tt, ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
        const int h0 = ty * 15 - 1, w0 = tx * 15 - 1, H2 = 2 * p.Ho, W2 = 2 * p.Wo;
        const int ylo = p.y_cpitch >> 1;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();                               // the last stage's fragment reads / the previous pass's window reads are done
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ni = pass * 2 + j;
                const float bb[4] = {bvA[ni].x, bvA[ni].y, bvA[ni].z, bvA[ni].w};
#pragma unroll
                for (int mi = 0; mi < FM; ++mi) {
                    half4 oh, ol;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[ni][mi][r] * p.pscale;
                        v += bb[r];
                        if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                        half_t a_, b_;
                        split_hl(v, a_, b_);
                        oh[r] = a_; ol[r] = b_;
                    }
                    const int chunk = j * 2 + (lg >> 1);   // 8-channel chunk (0..3) of this pass's 32 channels
                    char* px = img + mi * 2048 + lp * 128 + (lg & 1) * 8;
                    *reinterpret_cast<half4*>(px + ((chunk ^ (lp & 7)) << 4)) = oh;
                    *reinterpret_cast<half4*>(px + (((4 + chunk) ^ (lp & 7)) << 4)) = ol;
                }
            }
            __syncthreads();
            const int cbase = (n0 >> 2) + pass * 32;       // first output channel of this pass (64 output channels per 256-column tile)
            if (tid < 30 * 4 * 4 && (!p.cstore || cbase + (tid & 3) * 8 < p.cstore)) {
                const int ch = tid & 3, seg = (tid >> 2) & 3, Yl = tid >> 4;
                const int Y = 2 * (h0 + 1) + Yl;
                const int ay0 = max(Y - 1, 0);
                auto ld = [&](int ay, int ax, float (&f)[8]) {
                    const int dy = (ay >> 1) - h0, dx = (ax >> 1) - w0, q = (ay & 1) * 2 + (ax & 1);
                    const char* base = smem + ((dy >> 3) * WN + q) * (FM * 2048) + (dy & 7) * 2048 + dx * 128;
                    const half8 hi = *reinterpret_cast<const half8*>(base + ((ch ^ (dx & 7)) << 4));
                    const half8 lo = *reinterpret_cast<const half8*>(base + (((4 + ch) ^ (dx & 7)) << 4));
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = join_hl(hi[e], lo[e]);
                };
                if (Y < H2) {
                    const int xs = seg * 8 - (seg == 3 ? 1 : 0), cnt = seg < 2 ? 8 : 7;      // 30 columns = 8 + 8 + 7 + 7
                    const int X0 = 2 * (w0 + 1) + xs;
                    float l0[8], l1[8];                    // left column of the window (rows Y-1, Y)
                    {
                        const int axl = max(X0 - 1, 0);
                        ld(ay0, axl, l0);
                        ld(Y, axl, l1);
                    }
                    half_t* yrow = reinterpret_cast<half_t*>(p.y) + p.y_coff + cbase + ch * 8 + ((int64_t)(b * H2 + Y) * W2) * p.y_cpitch;
#pragma unroll 4
                    for (int k = 0; k < 8; ++k) {
                        const int X = X0 + k;
                        if (k >= cnt || X >= W2) break;
                        float r0[8], r1[8];
                        ld(ay0, X, r0);
                        ld(Y, X, r1);
                        half8 oh, ol;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float o = (l0[e] + r0[e] + l1[e] + r1[e]) * 0.25f;
                            half_t a_, b_;
                            split_hl(o, a_, b_);
                            oh[e] = a_; ol[e] = b_;
                        }
                        half_t* dstp = yrow + (int64_t)X * p.y_cpitch;
                        __builtin_nontemporal_store(oh, reinterpret_cast<half8*>(dstp));
                        __builtin_nontemporal_store(ol, reinterpret_cast<half8*>(dstp + ylo));
#pragma unroll
                        for (int e = 0; e < 8; ++e) { l0[e] = r0[e]; l1[e] = r1[e]; }
                    }
                }
            }
        }
        return;
    } else if (!lds_epi) {
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
            const int m = gm(wm * (FM * 16) + PF(mi) * 16 + lp);
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) epilogue_frag<PRECISE, UNIT_STEP && !PRECISE>(p, acc[ni][mi], m, n0 + wn * 64 + ni * 16 + lg * 4, HoWo, eflags);
        }
    } else if (EXTRA && has_extra && (eflags & HAVC_F_FUSE_RGB8)) {
        // ---- fused layers.11 (1x1 conv -> 3 channels) + SigmoidRange + denormalise + trunc u8 (HAVC_F_FUSE_RGB8) ----
        // r2 = fp16(ReLU(acc + bias) + residual) never leaves the registers: an accumulator fragment (lane = pixel lr,
        // channels lg*4..+3) IS the B operand of v_mfma_f32_16x16x16_f16, so the 1x1 conv is FN MFMAs per pixel
        // fragment with the (3 real of 16) output rows as A.  The 259-channel row of a pixel is spread over the four
        // N-waves and the extra-column fragments; the five partial sums go through LDS and are added in a FIXED
        // order, so a frame colours identically in any batch.
        fused_done = true;
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int nw0 = n0 + wn * 64;
        half4 wa[FN];
        float4 bvs[FN];
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const int n = nw0 + ni * 16 + lg * 4;
            wa[ni] = half4{0, 0, 0, 0};
            if (lr < 3) {
                const float4 w4 = *reinterpret_cast<const float4*>(p.fuse_w + lr * p.Npad + n);
                wa[ni] = half4{(half_t)w4.x, (half_t)w4.y, (half_t)w4.z, (half_t)w4.w};
            }
            bvs[ni] = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // extra columns: channels nx .. nx+2 are real (x0's RGB); lane group 0 folds this wave's two extra-column fragments into three partial dot
        // products per pixel.  Operands (bias, residual, fused weights: scalar loads, one dependent round trip) and arithmetic are split so that the
        // RES_LDS kernels request the operands with the first residual vectors instead of behind the projection.
        const int nx = n0 + BN;
        float xbias[4], xw[3][4], dx[2][3];
        half_t xres[2][4];
        auto extra_load = [&]() {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xbias[r] = p.bias ? p.bias[nx + r] : 0.f;
#pragma unroll
                for (int jo = 0; jo < 3; ++jo) xw[jo][r] = (float)(half_t)p.fuse_w[jo * p.Npad + nx + r];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = gm(wm * (FM * 16) + (wn * 2 + i) * 16 + lp);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xres[i][r] = (half_t)0.f;
                    if ((eflags & HAVC_F_RESIDUAL) && m < p.M && nx + r < p.Co) xres[i][r] = p.res[opix(m) * p.res_cpitch + p.res_coff + nx + r];
                }
            }
        };
        auto extra_fold = [&]() {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = gm(wm * (FM * 16) + (wn * 2 + i) * 16 + lp);
                float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = accx[i][r] + xbias[r];
                    if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                    if ((eflags & HAVC_F_RESIDUAL) && m < p.M && nx + r < p.Co)      // as epilogue_frag: fp16, then + residual
                        v = (float)(half_t)v + (float)xres[i][r];
                    const float f = (float)(half_t)v;
                    d0 += f * xw[0][r];
                    d1 += f * xw[1][r];
                    d2 += f * xw[2][r];
                }
                dx[i][0] = d0; dx[i][1] = d1; dx[i][2] = d2;
            }
        };
        // The residual (the 259-channel cat tensor: as many bytes as the conv reads).  RES_LDS, the compile-time-flag kernels: it takes the road of the
        // storing epilogue's phase 2, backwards: lane -> (pixel row lane>>3 (+8), 16-byte slot lane&7), so a wave's load touches 8 whole 128-byte lines
        // instead of 16 lines in 32-byte runs; the vectors go into the wave-private swizzled LDS image (the layout phase 1 of the storing epilogue
        // writes) and come back in fragment layout, one conflict-free ds_read_b64 per lane and column fragment.  Four pixel fragments (8 loads per
        // lane) at a time; the second four are requested before the first four are consumed.  Routing only: the operands and the order of every
        // addition are those of the direct loads.  The run-time-flag kernels and conv_halo_kernel (every layer kind's path in one register allocation:
        // the staging registers spill there) keep the direct half4 loads in fragment layout, four fragments in flight.
        constexpr bool RES_LDS = UNIT_STEP;
        const bool with_res = eflags & HAVC_F_RESIDUAL;
        const int rslot = lane & 7, rrow = lane >> 3;
        char* img = smem + wave * (FM * 2048);
        half8 rq[4][2];
#define HAVC_RES_FETCH(mh)                                                                                                              \
        _Pragma("unroll") for (int mj = 0; mj < 4; ++mj)                                                                                \
            _Pragma("unroll") for (int hp = 0; hp < 2; ++hp) {                                                                          \
                const int m = gm(wm * (FM * 16) + PF((mh) + mj) * 16 + rrow + hp * 8);                                                  \
                rq[mj][hp] = half8{0, 0, 0, 0, 0, 0, 0, 0};                                                                             \
                if (m < p.M) rq[mj][hp] = *reinterpret_cast<const half8*>(p.res + opix(m) * p.res_cpitch + p.res_coff + nw0 + rslot * 8); \
            }
#define HAVC_RES_STAGE(mh)                                                                                                              \
        _Pragma("unroll") for (int mj = 0; mj < 4; ++mj)                                                                                \
            _Pragma("unroll") for (int hp = 0; hp < 2; ++hp) {                                                                          \
                const int px = rrow + hp * 8;                                                                                           \
                *reinterpret_cast<half8*>(img + ((mh) + mj) * 2048 + px * 128 + ((rslot ^ (px & 7)) << 4)) = rq[mj][hp];                \
            }
        if (RES_LDS) {
            if (with_res) { HAVC_RES_FETCH(0) }
            if (lg == 0) extra_load();
            // every wave is done reading the last stage: the images may overwrite it.  Only the LDS reads have to be over -- __syncthreads() would also
            // drain the loads just requested (it waits for vmcnt 0 in front of the barrier)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        HAVC_STAMP(3);
        float4v facc[FM];
#pragma unroll
        for (int mh = 0; mh < FM; mh += 4) {
            half4 rd[4][FN];                               // !RES_LDS: four pixel fragments at a time, 16 residual loads in flight
            if (RES_LDS && with_res) {
                HAVC_RES_STAGE(mh)
                if (mh + 4 < FM) { HAVC_RES_FETCH(mh + 4) }
            }
            if (!RES_LDS) {
#pragma unroll
                for (int mj = 0; mj < 4; ++mj) {
                    const int m = gm(wm * (FM * 16) + PF(mh + mj) * 16 + lp);
#pragma unroll
                    for (int ni = 0; ni < FN; ++ni) {
                        rd[mj][ni] = half4{0, 0, 0, 0};
                        if (with_res && m < p.M)
                            rd[mj][ni] = *reinterpret_cast<const half4*>(p.res + opix(m) * p.res_cpitch + p.res_coff + nw0 + ni * 16 + lg * 4);
                    }
                }
            }
            if (mh == 0) HAVC_STAMP(10);
            if (RES_LDS && mh == 0 && lg == 0) extra_fold();
#pragma unroll
            for (int mj = 0; mj < 4; ++mj) {
                const int mi = mh + mj;
                half4 rr[FN];
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) {
                    if (!RES_LDS) rr[ni] = rd[mj][ni];
                    else if (with_res) rr[ni] = *reinterpret_cast<const half4*>(img + mi * 2048 + lp * 128 + (((ni * 2 + (lg >> 1)) ^ (lp & 7)) << 4) + (lg & 1) * 8);
                    else rr[ni] = half4{0, 0, 0, 0};
                }
                facc[mi] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) {
                    const float bb[4] = {bvs[ni].x, bvs[ni].y, bvs[ni].z, bvs[ni].w};
                    half4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[ni][mi][r] + bb[r];
                        if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                        o[r] = (half_t)((float)(half_t)v + (float)rr[ni][r]);    // the rounding points of the unfused chain (conv result -> fp16, + residual -> fp16)
                    }
                    facc[mi] = __builtin_amdgcn_mfma_f32_16x16x16f16(wa[ni], o, facc[mi], 0, 0, 0);
                }
            }
        }
#undef HAVC_RES_FETCH
#undef HAVC_RES_STAGE
        HAVC_STAMP(4);
        __syncthreads();                                   // every wave is done reading the last stage / its image: the reduction array below aliases both
        HAVC_STAMP(11);
        float* part = reinterpret_cast<float*>(smem);      // [5][BM][3]
        if (lg == 0) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                float* q = part + (wn * BM + wm * (FM * 16) + PF(mi) * 16 + lp) * 3;
                q[0] = facc[mi][0]; q[1] = facc[mi][1]; q[2] = facc[mi][2];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int pl = wm * (FM * 16) + (wn * 2 + i) * 16 + lp;
                if (!RES_LDS) {                            // operands fetched here, one by one (these kernels have no registers to hold them across the projection)
                    const int m = gm(pl);
                    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = accx[i][r] + (p.bias ? p.bias[nx + r] : 0.f);
                        if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                        if ((eflags & HAVC_F_RESIDUAL) && m < p.M && nx + r < p.Co)      // as epilogue_frag: fp16, then + residual
                            v = (float)(half_t)v + (float)p.res[opix(m) * p.res_cpitch + p.res_coff + nx + r];
                        const float f = (float)(half_t)v;
                        d0 += f * (float)(half_t)p.fuse_w[nx + r];
                        d1 += f * (float)(half_t)p.fuse_w[p.Npad + nx + r];
                        d2 += f * (float)(half_t)p.fuse_w[2 * p.Npad + nx + r];
                    }
                    dx[i][0] = d0; dx[i][1] = d1; dx[i][2] = d2;
                }
                float* q = part + (4 * BM + pl) * 3;
                q[0] = dx[i][0]; q[1] = dx[i][1]; q[2] = dx[i][2];
            }
        }
        __syncthreads();
        for (int pl = threadIdx.x; pl < BM; pl += NW * 64) {
            const int m = gm(pl);
            if (m >= p.M) continue;
            uint8_t* y = p.fuse_rgb + opix(m) * 3;
#pragma unroll
            for (int jo = 0; jo < 3; ++jo) {
                float t = p.fuse_b[jo];
#pragma unroll
                for (int w = 0; w < 5; ++w) t += part[(w * BM + pl) * 3 + jo];
                float sg = 1.f / (1.f + __expf(-t));
                sg = sg * (p.f1 - p.f0) + p.f0;
                sg = sg * p.istd[jo] + p.mean[jo];
                sg = fminf(fmaxf(sg, 0.f), 1.f);
                y[jo] = (uint8_t)(int)(sg * 255.f);
            }
        }
    } else if (!EXTRA && (eflags & HAVC_F_FUSE_PROJ) && WM == 2 && WN == 4 && FM == 8) {
        // ---- fused per-frame 256 -> 2 projection of this column tile (HAVC_F_FUSE_PROJ; DDColor: einsum + refine folded) ----
        // As the FUSE_RGB8 branch: an accumulator fragment (lane = pixel lr, channels lg*4..+3) is the B operand of
        // v_mfma_f32_16x16x16_f16 and the (2 real of 16) projection rows are A; the four N-waves' partial sums go through LDS
        // and are added in a fixed order.  The tile holds ONE column tile j = n0 / 256 of 256 pixels.
        fused_done = true;
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int nw0 = n0 + wn * 64, cw0 = wn * 64;       // channel within the column tile: the projection repeats per tile
        float4 bvs[FN];
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
            bvs[ni] = p.bias ? *reinterpret_cast<const float4*>(p.bias + nw0 + ni * 16 + lg * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4v facc[FM];
        int fb_prev = -1;
        half4 wa[FN];
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
            const int mf = gm(wm * (FM * 16) + mi * 16);    // a 16-pixel fragment lies in one frame (Ho * Wo % 16 == 0)
            const int fb = mf < p.M ? (int)fast_div((unsigned)mf, p.fd_howo) : 0;
            if (fb != fb_prev) {
                fb_prev = fb;
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) {
                    wa[ni] = half4{0, 0, 0, 0};
                    if (lr < 2) {
                        const float4 w4 = *reinterpret_cast<const float4*>(p.fuse_w + ((size_t)fb * 2 + lr) * 256 + cw0 + ni * 16 + lg * 4);
                        wa[ni] = half4{(half_t)w4.x, (half_t)w4.y, (half_t)w4.z, (half_t)w4.w};
                    }
                }
            }
            facc[mi] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) {
                const float bb[4] = {bvs[ni].x, bvs[ni].y, bvs[ni].z, bvs[ni].w};
                half4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[ni][mi][r] + bb[r];
                    if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                    o[r] = (half_t)v;                      // the value the unfused chain stores
                }
                facc[mi] = __builtin_amdgcn_mfma_f32_16x16x16f16(wa[ni], o, facc[mi], 0, 0, 0);
            }
        }
        __syncthreads();                                   // every wave is done reading the last stage
        float* part = reinterpret_cast<float*>(smem);      // [4][BM][2]
        if (lg == 0) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                float* q = part + (wn * BM + wm * (FM * 16) + mi * 16 + lp) * 2;
                q[0] = facc[mi][0]; q[1] = facc[mi][1];
            }
        }
        __syncthreads();
        const int NTp = p.Npad >> 8, jt = n0 >> 8;
        for (int pl = threadIdx.x; pl < BM; pl += NW * 64) {
            const int m = gm(pl);
            if (m >= p.M) continue;
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { t0 += part[(w * BM + pl) * 2]; t1 += part[(w * BM + pl) * 2 + 1]; }
            *reinterpret_cast<float2*>(p.fuse_out + ((size_t)m * NTp + jt) * 2) = make_float2(t0, t1);
        }
    } else {
        const bool leaky = eflags & HAVC_F_LEAKY;
        const int nw0 = n0 + wn * 64;                      // first channel of this wave's 64-channel slice
        // bias / scale / shift of all four column fragments requested at once and BEFORE the barrier: inside the fragment loop each load was
        // followed by its own s_waitcnt vmcnt(0) -- four (twelve with AFFINE) serialised L2 round trips per tile (round 4)
        float4 bvA[FN], scA[FN], shA[FN];
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const int n = nw0 + ni * 16 + lg * 4;
            const bool n_ok = n < p.Npad;
            bvA[ni] = make_float4(0.f, 0.f, 0.f, 0.f); scA[ni] = make_float4(1.f, 1.f, 1.f, 1.f); shA[ni] = bvA[ni];
            if (p.bias && n_ok) bvA[ni] = *reinterpret_cast<const float4*>(p.bias + n);
            if ((eflags & HAVC_F_AFFINE) && n_ok) {
                scA[ni] = *reinterpret_cast<const float4*>(p.scale + n);
                shA[ni] = *reinterpret_cast<const float4*>(p.shift + n);
            }
        }
        __syncthreads();                                   // every wave is done reading the last stage
        HAVC_STAMP(3);
        char* img = smem + wave * (FM * 2048);
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const float4 bv = bvA[ni], sc = scA[ni], sh = shA[ni];
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w}, ss[4] = {sc.x, sc.y, sc.z, sc.w}, hh[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                half4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[ni][mi][r] + bb[r];
                    if (eflags & HAVC_F_RELU_PRE) v = v > 0.f ? v : (leaky ? v * p.f2 : 0.f);
                    if (eflags & HAVC_F_GELU) v = gelu_erf(v);
                    if (eflags & HAVC_F_AFFINE) v = v * ss[r] + hh[r];
                    o[r] = (half_t)v;
                }
                const int slot = (ni * 2 + (lg >> 1)) ^ (lp & 7);
                *reinterpret_cast<half4*>(img + mi * 2048 + lp * 128 + slot * 16 + (lg & 1) * 8) = o;
            }
        }
        if ((eflags & HAVC_F_PS_BLUR) && WM == 2 && WN == 4 && FM == 8) {
            // ---- HAVC_F_PS_BLUR: PixelShuffle(2) + ReplicationPad(1,0,1,0) + AvgPool2d(2,1) straight out of the LDS images ----
            // The block holds the 16x16 low-res tile x (4 sub-pixels x 64 channels); wave (wm, q) owns rows wm*8..+7 of
            // sub-pixel q.  Output = the 30x30 hi-res pixels whose 2x2 source window lies inside the tile.  Same fp16
            // rounding of the shuffled values and the same summation order as elementwise.hip blur_resize_kernel.
            __syncthreads();
            const int tile = m0 / BM, tt = p.tiles_y * p.tiles_x;
            const int b = (int)fast_div((unsigned)tile, p.fd_tt), t = tile - b * tt, ty = (int)fast_div((unsigned)t, p.fd_tx), tx = t - ty * p.tiles_x;
            const int h0 = ty * 15 - 1, w0 = tx * 15 - 1, H2 = 2 * p.Ho, W2 = 2 * p.Wo;
            half_t* y = reinterpret_cast<half_t*>(p.y) + p.y_coff + (n0 >> 2);          // 64 output channels per 256-column tile
            // Thread (row Yl of the 30 x 30 output tile, half xh of the row, 16-byte channel chunk ch) walks 15 consecutive output
            // columns: the 2 x 2 window slides by one column per output, so the right-hand column of one output is the left-hand
            // column of the next and only TWO LDS reads (rows Y-1, Y of the new column) + their fp32 conversions are needed per
            // output instead of four (the epilogue's arithmetic was ~1/3 of this kernel).  Same operands, same order of the fp32
            // adds ((v00 + v01) + v10) + v11 as blur_resize_kernel: bit-identical.  Stores are non-temporal: the tensor (2.6 GB per
            // 16 frames at 560^2) is far beyond the Infinity Cache and is next read by another kernel.
            if (tid < 30 * 2 * 8 && (!p.cstore || (n0 >> 2) + (tid & 7) * 8 < p.cstore)) {      // chunks beyond the stored channels: zero pad rows
                const int ch = tid & 7, xh = (tid >> 3) & 1, Yl = tid >> 4;
                const int Y = 2 * (h0 + 1) + Yl;
                const int ay0 = max(Y - 1, 0);
                auto ld = [&](int ay, int ax) -> half8 {
                    const int dy = (ay >> 1) - h0, dx = (ax >> 1) - w0, q = (ay & 1) * 2 + (ax & 1);
                    return *reinterpret_cast<const half8*>(smem + ((dy >> 3) * WN + q) * (FM * 2048) + (dy & 7) * 2048 + dx * 128 + ((ch ^ (dx & 7)) << 4));
                };
                if (Y < H2) {
                    const int X0 = 2 * (w0 + 1) + xh * 15;
                    float l0[8], l1[8];                                  // left column of the window (rows Y-1, Y), fp32
                    {
                        const int axl = max(X0 - 1, 0);
                        const half8 a = ld(ay0, axl), c = ld(Y, axl);
#pragma unroll
                        for (int e = 0; e < 8; ++e) { l0[e] = (float)a[e]; l1[e] = (float)c[e]; }
                    }
                    half_t* yrow = y + ((int64_t)(b * H2 + Y) * W2) * p.y_cpitch + ch * 8;
#pragma unroll 5
                    for (int k = 0; k < 15; ++k) {
                        const int X = X0 + k;
                        if (X >= W2) break;
                        const half8 a = ld(ay0, X), c = ld(Y, X);
                        half8 o;
                        float r0[8], r1[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            r0[e] = (float)a[e]; r1[e] = (float)c[e];
                            o[e] = (half_t)((l0[e] + r0[e] + l1[e] + r1[e]) * 0.25f);
                        }
                        // X == 0 replicates the column (ReplicationPad left): the "left" column of output 0 is column 0 itself
                        half8* dstp = reinterpret_cast<half8*>(yrow + (int64_t)X * p.y_cpitch);
                        if (ABL == 11) { if (o[0] == (half_t)123.f && o[1] == (half_t)77.f) *dstp = o; }       // profiling: compute, (almost) no stores
                        else if (ABL == 13) *dstp = o;                                                          // profiling: plain stores
                        else __builtin_nontemporal_store(o, dstp);
#pragma unroll
                        for (int e = 0; e < 8; ++e) { l0[e] = r0[e]; l1[e] = r1[e]; }
                    }
                }
            }
            return;
        }
        HAVC_STAMP(4);
        // phase 2: lane -> (pixel row lane>>3 (+8), 16-byte channel slot lane&7).  All residual vectors are requested
        // up front (the accumulators are dead by now) so their latency overlaps instead of serialising 16 load->store pairs.
        const int ch = lane & 7;
        const int n = nw0 + ch * 8;
        const bool do_res = (eflags & HAVC_F_RESIDUAL) && !(eflags & HAVC_F_OUT_PIXSHUF) && n < p.Co;
        half8 rres[FM][2];
        if (eflags & HAVC_F_RESIDUAL) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi)
#pragma unroll
                for (int hp = 0; hp < 2; ++hp) {
                    const int m = gm(wm * (FM * 16) + PF(mi) * 16 + (lane >> 3) + hp * 8);
                    rres[mi][hp] = half8{0, 0, 0, 0, 0, 0, 0, 0};
                    if (do_res && m < p.M) rres[mi][hp] = *reinterpret_cast<const half8*>(p.res + opix(m) * p.res_cpitch + p.res_coff + n);
                }
        }
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
#pragma unroll
            for (int hp = 0; hp < 2; ++hp) {
                const int px = (lane >> 3) + hp * 8;
                const int m = gm(wm * (FM * 16) + PF(mi) * 16 + px);
                const half8 v = *reinterpret_cast<const half8*>(img + mi * 2048 + px * 128 + ((ch ^ (px & 7)) << 4));
                if (m >= p.M) continue;
                half_t* y = reinterpret_cast<half_t*>(p.y);
                int64_t off;
                if (eflags & HAVC_F_OUT_PIXSHUF) {
                    const int q = n / p.Co, cc = n - q * p.Co;
                    if (q >= 4) continue;
                    const int b = (int)fast_div((unsigned)m, p.fd_howo), rem = m - b * HoWo, ho = (int)fast_div((unsigned)rem, p.fd_wo), wo = rem - ho * p.Wo;
                    off =((int64_t)(b * 2 * p.Ho + 2 * ho + (q >> 1)) * (2 * p.Wo) + 2 * wo + (q & 1)) * p.y_cpitch + p.y_coff + cc;
                } else {
                    if (n >= p.Co) continue;
                    off = opix(m) * p.y_cpitch + p.y_coff + n;
                }
                half8 o = v;
                if (eflags & (HAVC_F_RESIDUAL | HAVC_F_RELU_POST)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float f = (float)v[e];
                        if (eflags & HAVC_F_RESIDUAL) f += (float)rres[mi][hp][e];
                        if (eflags & HAVC_F_RELU_POST) f = f > 0.f ? f : (leaky ? f * p.f2 : 0.f);
                        o[e] = (half_t)f;
                    }
                }
                if (ABL == 12) { if (o[0] == (half_t)123.f && o[1] == (half_t)77.f) *reinterpret_cast<half8*>(y + off) = o; }   // profiling: (almost) no stores
                else if (ABL == 14) *reinterpret_cast<half8*>(y + (off & 0xFFFF8)) = o;                                        // profiling: every store inside one 2-MiB window
                else if (eflags & HAVC_F_NT_STORE) __builtin_nontemporal_store(o, reinterpret_cast<half8*>(y + off));
                else *reinterpret_cast<half8*>(y + off) = o;
            }
        }
    }
    if (EXTRA && has_extra && !(fused_done)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = gm(wm * (FM * 16) + (wn * 2 + i) * 16 + lp);
            epilogue_frag<PRECISE, UNIT_STEP && !PRECISE>(p, accx[i], m, n0 + BN + lg * 4, HoWo, eflags);
        }
    }
