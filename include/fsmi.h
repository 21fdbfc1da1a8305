/*
 * fsmi.h -- C ABI of libfsmi.so, the MI355X-native (gfx950) hot path of
 * FoundationStereo: cost-volume build, geometry encoding, per-iteration
 * correlation lookup, soft-argmin, convex upsampling and ConvGRU gates.
 *
 * Conventions (every entry point):
 *   - all tensors are fp32, contiguous, row-major, already resident in device
 *     memory (HBM); pointers are device pointers, shapes are plain ints;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are asynchronous on that stream, nothing allocates, nothing
 *     synchronises, so every call is hipGraph-capturable;
 *   - return 0 on success, FSMI_ERR_ARG (1001) when an argument violates the
 *     contract (message in fsmi_last_error()), or the hipError_t of a failed
 *     launch.
 *
 * Reference interfaces replaced are cited as path:line in TongZhe2016/
 * FoundationStereo (snapshot 2025-06-29).  See INTEGRATION.md for bindings.
 */
#ifndef FSMI_H_
#define FSMI_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSMI_OK 0
#define FSMI_ERR_ARG 1001
#define FSMI_MAX_LEVELS 4

/* ---- library ---------------------------------------------------------- */
int fsmi_version(void);                /* 100*major + minor */
const char* fsmi_last_error(void);     /* thread-local, "" when none */
const char* fsmi_arch(void);           /* "gfx950" */

/* ---- a1: group-wise correlation volume --------------------------------
 * replaces build_gwc_volume / groupwise_correlation, core/submodule.py:388-412
 * fl, fr: (B,C,H,W); out: (B,G,D,H,W).  out[b,g,d,h,w] = <nL,nR(w-d)> over
 * the C/G channels of group g after L2 normalisation (eps 1e-12), 0 for w<d.
 * Requires C % G == 0 (reference: AssertionError at core/submodule.py:390). */
int fsmi_gwc_volume(const float* fl, const float* fr, float* out,
                    int B, int C, int G, int D, int H, int W, void* stream);

/* ---- a2: concat volume -------------------------------------------------
 * replaces build_concat_volume, core/submodule.py:416-427
 * pl, pr: (B,C,H,W); out: (B,2C,D,H,W): left half copied for all w, right
 * half shifted by d and zero for w<d. */
int fsmi_concat_volume(const float* pl, const float* pr, float* out,
                       int B, int C, int D, int H, int W, void* stream);

/* ---- a1+a2+corr_stem[0] fused ------------------------------------------
 * replaces core/foundation_stereo.py:207-213 up to and including the
 * 1x1x1 Conv3d(32 -> Cs) of corr_stem (core/foundation_stereo.py:165):
 *   out[b,o,d,h,w] = A[b,o,h,w] + [w>=d] Bm[b,o,h,w-d] + sum_g Wg[o,g] gwc[b,g,d,h,w]
 * where A, Bm: (B,Cs,H,W) are the proj_cmb features already multiplied by the
 * concat columns of the stem weight (A also carries the stem bias), and
 * Wg: (Cs,G) the gwc columns.  out: (B,Cs,D,H,W).  gwc_ws: optional
 * (B,G,D,H,W) scratch; with it the build runs as two streaming passes (gwc
 * tile kernel, then the stem stream), without it as one LDS-staged kernel. */
int fsmi_comb_volume_stem(const float* fl, const float* fr, const float* A, const float* Bm,
                          const float* Wg, float* gwc_ws, float* out,
                          int B, int C, int G, int Cs, int D, int H, int W, void* stream);

/* pointwise 2-output projection used to form A / Bm above:
 * out[b,o,h,w] = bias[o] + sum_c Wt[o,c] x[b,c,h,w];  x: (B,C,H,W), out: (B,O,H,W) */
int fsmi_pointwise_proj(const float* x, const float* Wt, const float* bias, float* out,
                        int B, int C, int O, int H, int W, void* stream);

/* ---- a5: all-pairs correlation + W2 pyramid (fp32 MFMA) ----------------
 * replaces Combined_Geo_Encoding_Volume.corr + its avg-pool pyramid,
 * core/geometry.py:24-40,68-77.  fl, fr: (B,C,H,W).  levels[i]: (B,H,W,W>>i')
 * with W_i = floor(W_{i-1}/2); level 0 is the full (B,H,W1,W2) correlation of
 * the channel-L2-normalised features.  ws: optional 2*B*C*H*W-float scratch;
 * with it the features are normalised once and the MFMA pass reads them
 * straight from L2, without it one LDS-staged kernel normalises per block. */
int fsmi_allpairs_corr(const float* fl, const float* fr, float* const* levels, int num_levels,
                       int B, int C, int H, int W, float* ws, void* stream);

/* ---- a5: filtered-volume pyramid over D ---------------------------------
 * replaces core/geometry.py:29,34-36 without the permute copy.  vol:
 * (B,Cv,D,H,W) native layout; levels[i-1]: (B,Cv,D_i,H,W), i=1..num_levels-1,
 * D_i = floor(D_{i-1}/2), value = mean of the two parents (iterated). */
int fsmi_volume_pyramid(const float* vol, float* const* levels, int num_levels,
                        int B, int Cv, int D, int H, int W, void* stream);

/* ---- a6: per-iteration multi-level lookup ------------------------------
 * replaces Combined_Geo_Encoding_Volume.__call__ + bilinear_sampler,
 * core/geometry.py:43-65, core/utils/utils.py:44-55.
 * vol_levels[i]: (B,Cv,D_i,H,W); corr_levels[i]: (B,H,W,W2_i); disp: (B,1,H,W);
 * out: (B, L*(2r+1)*(Cv+1), H, W) with channel order per level
 * [geo (c*(2r+1)+k) ..., corr k ...] (core/geometry.py:62-65).
 * Taps at x = disp/2^i + k and x = w/2^i - disp/2^i + k, k in [-r,r]; linear
 * interpolation, align_corners=True, zero padding.  Requires D_i >= 2, W2_i >= 2. */
int fsmi_geo_lookup(const float* const* vol_levels, const float* const* corr_levels,
                    const float* disp, float* out,
                    int num_levels, int radius, int B, int Cv, int D, int H, int W, int W2,
                    void* stream);
/* the same with the reference's `coords` argument (core/geometry.py:43,57): coords (B,H,W) fp32, the
 * column coordinate of each pixel on the left image (core/foundation_stereo.py:231 passes arange(W)
 * per row), so the corr taps sit at x = coords/2^i - disp/2^i + k.  coords == NULL: the pixel column
 * w (what fsmi_geo_lookup does, without the load). */
int fsmi_geo_lookup_coords(const float* const* vol_levels, const float* const* corr_levels,
                           const float* disp, const float* coords, float* out,
                           int num_levels, int radius, int B, int Cv, int D, int H, int W, int W2,
                           void* stream);

/* 1-D stereo specialisation of bilinear_sampler (core/utils/utils.py:44-55):
 * img (P,C,1,Lx); x (P,K) pixel x-coordinates (y == 0); out (P,C,1,K). */
int fsmi_bilinear_sampler_1d(const float* img, const float* x, float* out,
                             int P, int C, int Lx, int K, void* stream);

/* ---- a4: soft-argmin ---------------------------------------------------
 * fsmi_disparity_regression: core/submodule.py:431-435, prob (B,D,H,W) -> (B,1,H,W)
 * fsmi_softmax_regression:  core/foundation_stereo.py:218-220 fused
 *                           (softmax over D of logits, then sum d*p_d). */
int fsmi_disparity_regression(const float* prob, float* out, int B, int D, int H, int W, void* stream);
int fsmi_softmax_regression(const float* logits, float* out, int B, int D, int H, int W, void* stream);

/* ---- a9: convex upsampling ---------------------------------------------
 * fsmi_context_upsample: core/submodule.py:456-468; disp (B,1,h,w),
 *   w (B,9,4h,4w) -> out (B,4h,4w).
 * fsmi_softmax_context_upsample: core/foundation_stereo.py:187-189 fused:
 *   softmax over the 9 logits, scale disp by `scale` (4.0), convex combine. */
int fsmi_context_upsample(const float* disp, const float* w, float* out, int B, int h, int w_, void* stream);
int fsmi_softmax_context_upsample(const float* disp, const float* logits, float* out, float scale,
                                  int B, int h, int w_, void* stream);

/* ---- a7: selective ConvGRU gates (core/update.py:83-119) ----------------
 * zr_s / zr_l: (B, 2*Hd, H, W) pre-activations [z | r] of the small (k=1) and
 * large (k=3) RaftConvGRU; h: (B,Hd,H,W); x: (B,Cx,H,W).
 * fsmi_gru_reset: qin_s/qin_l (B, Hd+Cx, H, W) <- [sigmoid(r)*h , x]   (update.py:92-93)
 * fsmi_gru_blend: hout <- att*((1-zs)h+zs*tanh(qs)) + (1-att)*((1-zl)h+zl*tanh(ql))
 *                 with z = sigmoid(z_pre); q_s/q_l: (B,Hd,H,W); att (B,1,H,W);
 *                 (update.py:91,94-95,117). hout may alias h. */
int fsmi_gru_reset(const float* zr_s, const float* zr_l, const float* h, const float* x,
                   float* qin_s, float* qin_l, int B, int Hd, int Cx, int H, int W, void* stream);
int fsmi_gru_blend(const float* zr_s, const float* zr_l, const float* q_s, const float* q_l,
                   const float* h, const float* att, float* hout,
                   int B, int Hd, int H, int W, void* stream);

/* ---- a3: few-output-channel direct 3D convolution ------------------------
 * replaces the classifier's final nn.Conv3d(14, 1, kernel_size=7, padding=3)
 * (core/foundation_stereo.py:175): x (B,Cin,D,H,W), w (Cout,Cin,KS,KS,KS),
 * bias (Cout) or NULL -> out (B,Cout,D,H,W); stride 1, zero padding KS/2.
 * Supported (KS, Cout): (7,1), (3,1). */
int fsmi_conv3d_direct(const float* x, const float* w, const float* bias, float* out,
                       int B, int Cin, int Cout, int KS, int D, int H, int W, void* stream);

/* Convolution of the refinement loop, halo-tiled split-precision MFMA.
 * replaces the nn.Conv2d / nn.Linear stacks of the refinement loop
 * (core/update.py:20-159: motion encoder, SelectiveConvGRU convs, DispHead,
 * mask head) plus the elementwise passes that follow them.
 * Input: nseg NCHW channel segments concatenated along C (zero-copy cat):
 *   segment i = seg_ch[i] channels starting at seg_ptr[i] inside a tensor with
 *   seg_ctot[i] channels per image (batch stride seg_ctot[i]*H*W).
 * out[b, co0+co] (tensor with out_ctot channels) =
 *   res[b,co] + gamma[co] * alpha * act(conv + bias[co]);  act 0 none, 1 ReLU, 2 GELU(erf),
 *   6 LeakyReLU 0.01; gamma/res may be NULL (res has res_ctot channels per image).
 *   act 7: out = ReLU(conv + bias[co] + res[b,co]) (res required, gamma NULL, alpha 1): the
 *   remaining input channels of a conv whose loop-invariant channels were convolved once
 *   into res (SelectiveConvGRU.conv0's context segment, core/update.py:112-113).
 * Split-precision operands on the fp16 MFMA ("3 x fp16"): x = hi + lo (two fp16),
 * product = hi*hi + hi*lo + lo*hi accumulated in fp32 (~22-bit operands).  whi/wlo:
 * _Float16 weights packed [KS*KS][Cin32/32][Cout32][32] (Cin32/Cout32 = Cin/Cout rounded
 * up to 32, zero padded).  Square KS in {1, 3}.  Range-safe split: each output channel's weights are packed
 * x 2^wexp[co] (its max |w| in [1, 2)); scale_bias (2*Cout floats, device, 8-B
 * aligned) holds the pairs (2^-wexp[co], bias[co]) the epilogue applies as
 * conv * scale + bias; activations get a block exponent per 32-channel chunk in the
 * kernel (conv_halo.h, chunk_exp), so neither overflows fp16 nor loses its low
 * half to fp16 subnormals.  A block stages a (rows+2)x34 input halo once per
 * 32-channel chunk and runs all taps from LDS.  Inner segments must hold a
 * multiple of 8 channels.  cfg names the tile, couts x (rows x 32 px), of the table csrc/conv_tiles.h:
 *   c (0..11): halo tile c (0 / 1 stage weights per tap through LDS, the others keep each wave's
 *     weight fragments in registers, loaded one tap ahead; 10 is stride 2 only, 11 2D only);
 *   16 + c: tile c with two K groups -- 512-thread blocks whose two wave groups take
 *     alternate 32-channel chunks and sum through LDS (split-K inside the block);
 *   24..29: the pointwise LDS-DMA tiles (2D 1x1 layers, H*W % 4 == 0, 16-B aligned segments);
 *   30: the depth-blocked tile ((17,1,1) volume convs);
 *   32 + c: register-weight tile c with pipelined staging (2D maps; a volume runs tile c);
 *   -1: measured default.  A cfg the table does not give the conv is FSMI_ERR_ARG.
 * nsplit: split-K over 32-channel chunks (<0: auto, sized to fill the chip);
 * partial sums go to ws (nsplit*B*Cout*H*W floats, ws_floats available) and
 * a second kernel sums them in split order (deterministic) and applies the
 * epilogue.  ws may be NULL when nsplit is 0/1 (or auto: then no split).
 * (A last-arriving-block fixup inside the conv kernel was measured 4x slower:
 * the agent-scope fences it needs flush and invalidate the per-XCD L2.) */
/* Launches of the halo / pointwise / depth conv tiles since the last reset, per tile config as
 * launched: counts[c] for c < n (n <= 64), c in the cfg encoding of fsmi_conv2d_halo_x3 below
 * (csrc/conv_tiles.h).  reset != 0 zeroes them after the read.  (Which tile the tuning table
 * or the policy picked for a layer, checked by tests.) */
int fsmi_conv_launch_counts(long long* counts, int n, int reset);

int fsmi_conv2d_halo_x3(const float* const* seg_ptr, const int* seg_ch, const int* seg_ctot, int nseg,
                        const void* whi, const void* wlo, const float* scale_bias, const float* gamma,
                        const float* res, int res_ctot, float* out, int out_ctot, int co0, int B, int Cout,
                        int KS, int H, int W, int act, float alpha, int cfg, int nsplit, float* ws,
                        long long ws_floats, void* stream);

/* The same halo conv with a SelectiveConvGRU gate as its epilogue (replaces
 * the gate elementwise passes of core/update.py:88-95,117; Hd = hidden channels,
 * h / z / rh / out (B,Hd,H,W), att (B,1,H,W), all written/read in place):
 *   mode 0 (convz|convr stacked, Cout = 2Hd): z = sigmoid(conv[:Hd]),
 *          rh = sigmoid(conv[Hd:]) * h   (rh then feeds convq as a segment beside x);
 *   mode 1 (small GRU convq, Cout = Hd): out[:, co0:] = ((1-z)h + z tanh(conv)) * att;
 *   mode 2 (large GRU convq):            out[:, co0:] += ((1-z)h + z tanh(conv)) * (1-att).
 * conv includes the bias.  Other arguments as fsmi_conv2d_halo_x3. */
int fsmi_conv2d_halo_x3_gate(const float* const* seg_ptr, const int* seg_ch, const int* seg_ctot, int nseg,
                             const void* whi, const void* wlo, const float* scale_bias, int mode,
                             const float* h, float* z, const float* att, float* rh, int Hd, float* out,
                             int out_ctot, int co0, int B, int Cout, int KS, int H, int W, int cfg, int nsplit,
                             float* ws, long long ws_floats, void* stream);

/* ---- a3: 3D cost filtering (stride-1 Conv3d + folded BatchNorm) ----------
 * replaces the stride-1 Conv3d+BN(+act) layers of core/submodule.py:51-195
 * (BasicConv, Conv3dNormActReduced, ResnetBasicBlock3D) on MIOpen.  The same
 * halo split-precision kernel: a KD x KS x KS conv (KS in {1,3}, KD odd, zero
 * padding KD/2, KS/2) is the sum over kd of 2D convs on depth plane d+kd-KD/2.
 * x (B,Cin,D,H,W), out / res (B,Cout,D,H,W); whi/wlo packed as for
 * fsmi_conv2d_halo_x3 with taps = (kd, kh, kw), kd major; bias = folded conv bias +
 * BatchNorm shift.  out = act(conv + bias) + res, or with res_pre
 * act(conv + bias + res); act 0 none, 1 ReLU, 6 LeakyReLU(0.01).
 * cfg as fsmi_conv2d_halo_x3 (no 2D-only or pointwise tile on a volume). */
int fsmi_conv3d_halo_x3(const float* x, int Cin, const void* whi, const void* wlo, const float* scale_bias,
                        const float* res, float* out, int B, int Cout, int D, int H, int W, int KD, int KS,
                        int act, int res_pre, int cfg, int nsplit, float* ws, long long ws_floats, void* stream);

/* ---- a3: stride-2 Conv3d and the fused FeatureAtt gate ----------------------
 * fsmi_conv3d_halo_x3 with two more terms:
 *   stride 2: the hourglass BasicConv(is_3d, kernel_size=3, stride=2, padding=1) + BN + LeakyReLU
 *     (core/foundation_stereo.py:50-58), and with D = KD = 1 the context net's 3x3 s2 p1 convs and
 *     1x1 s2 projections (core/extractor.py:20-80): KS, KD in {1, 3} with padding KS/2, KD/2;
 *     D, H, W are the INPUT's, out / res are (B, Cout, (D-1)/2+1, (H-1)/2+1, (W-1)/2+1); cfg -1 or
 *     one of the table's stride-2 tiles (4, 5, 7, 10).
 *   res_pre needs a volume (D or KD > 1) or stride 2 (FSMI_ERR_ARG otherwise).
 *   fatt: FeatureAtt (core/submodule.py:438-454) folded into the epilogue -- the final value of
 *     output channel co at (d, h, w) is multiplied by sigmoid(fatt[b, co, h, w]); fatt is the
 *     gate's pre-sigmoid (B, Cout, Ho, Wo) map (contiguous) or NULL. */
int fsmi_conv3d_halo_x3_ex(const float* x, int Cin, const void* whi, const void* wlo, const float* scale_bias,
                           const float* res, const float* fatt, float* out, int B, int Cout, int D, int H, int W,
                           int KD, int KS, int stride, int act, int res_pre, int cfg, int nsplit, float* ws,
                           long long ws_floats, void* stream);

/* ---- refinement-loop auxiliaries ---------------------------------------
 * fsmi_dwconv2d: depthwise KSxKS conv (KS in {3,5,7}, stride 1, zero pad KS/2)
 *   x, out (B,C,H,W); w (C,1,KS,KS); bias (C) or NULL.  Replaces the EdgeNeXt
 *   dwconv of DispHead (core/submodule.py:565-591 via core/update.py:24-31).
 * fsmi_resize_bilinear: F.interpolate(x, (Ho,Wo), mode="bilinear",
 *   align_corners=True) on (B,C,Hi,Wi) -> (B,C,Ho,Wo) (interp, core/update.py:80). */
/* ---- a3: ConvTranspose3d(k=4, s=2, p=1) + folded BatchNorm + activation -------------
 * replaces the hourglass *_up BasicConv(deconv=True, is_3d=True), core/foundation_stereo.py:62-68
 * with core/submodule.py:51-86: x (B,Cin,D,H,W) -> out (B,Cout,2D,2H,2W).  Output phase
 * p = 4*pd + 2*ph + pw (voxels (2d+pd, 2h+ph, 2w+pw)) is a 2x2x2 stride-1 conv over x:
 * whi[p] / wlo[p] packed as fsmi_conv3d_halo_x3's weights (KD = KS = 2, taps at input offsets
 * {-1, 0} for phase 0 and {0, +1} for phase 1 of each dimension; ops.pack_deconv_phases),
 * scale_bias[p] its (2^-wexp, bias) pairs.  act 0 none / 1 ReLU / 6 LeakyReLU(0.01); cfg one of
 * the table's transposed-conv phase tiles (2, 3, 5, 6, 7) or -1. */
int fsmi_conv3d_up2_halo_x3(const float* x, int Cin, const void* const* whi, const void* const* wlo,
                            const float* const* scale_bias, float* out, int B, int Cout, int D, int H, int W,
                            int act, int cfg, void* stream);
/* ConvTranspose2d(k=4, s=2, p=1) (+ bias / folded BN, activation 0 / 1 ReLU / 6 LeakyReLU) on 2x2
 * phase tiles: x (B,Cin,H,W) -> out (B,Cout,2H,2W); whi / wlo / scale_bias: the 4 phase packs
 * (phase p = 2*oh + ow writes output pixels (2h + oh, 2w + ow)).  Replaces the spx upsampling
 * deconvs spx_2_gru.conv1 and spx_gru (core/foundation_stereo.py:183-191, core/submodule.py:281-317). */
int fsmi_conv2d_up2_halo_x3(const float* x, int Cin, const void* const* whi, const void* const* wlo,
                            const float* const* scale_bias, float* out, int B, int Cout, int H, int W,
                            int act, int cfg, void* stream);

int fsmi_dwconv2d(const float* x, const float* w, const float* bias, float* out, int B, int C, int KS,
                  int H, int W, void* stream);
/* fsmi_edgenext_mlp: the inverted-bottleneck MLP of EdgeNextConvEncoder (core/submodule.py:583-590,
 *   replacing pwconv1 -> GELU -> pwconv2 -> gamma -> residual):
 *   out[b,:,p] = res[b,:,p] + gamma * (W2 gelu(W1 x[b,:,p] + b1) + b2), x / res / out (B,C,H,W)
 *   (out may alias res, not x); w1hi/w1lo = ops.PackedConv of W1 (E x C) as a 1x1 conv,
 *   sb1 its (2^-wexp, b1) pairs (E float2), w2hi/w2lo / sb2 the same for W2 (C x E); gamma (C) or
 *   NULL.  Split-precision MFMA (3 fp16 products per MAC) with fp32 accumulation; the 4C hidden
 *   map stays in LDS.  Built for C = 128, E = 4C (DispHead). */
int fsmi_edgenext_mlp(const float* x, const float* res, float* out, const void* w1hi, const void* w1lo,
                      const float* sb1, const void* w2hi, const void* w2lo, const float* sb2, const float* gamma,
                      int B, int C, int E, int H, int W, void* stream);
int fsmi_resize_bilinear(const float* x, float* out, int B, int C, int Hi, int Wi, int Ho, int Wo, void* stream);
/* fsmi_conv3x3_cout1: Conv2d(Cin, 1, 3, padding=1) + bias (+ res) in fp32 on (B,Cin,H,W) (dense NCHW):
 * out[b*out_bstride + p] = res[b*res_bstride + p] + bias[0] + sum_c,tap w[c*9 + tap] * x[b, c, p + tap];
 * bias (device, 1 float) and res may be NULL.  DispHead's last layer (core/update.py:28), whose caller adds disp (the loop's
 * disp + delta, core/foundation_stereo.py:240-241) and writes it into the next motion-feature buffer. */
int fsmi_conv3x3_cout1(const float* x, int Cin, const float* w, const float* bias, const float* res, long long res_bstride,
                       float* out, long long out_bstride, int B, int H, int W, void* stream);

/* fsmi_conv2d_1in: Conv2d(1, Cout, KS, padding=KS//2) (+ ReLU when relu != 0) on (B,1,H,W) ->
 *   (B,Cout,H,W): the motion encoder's convd1 + ReLU (core/update.py:57,67); KS in {3,5,7}. */
int fsmi_conv2d_1in(const float* x, const float* w, const float* bias, float* out, int B, int Cout, int KS,
                    int H, int W, int relu, void* stream);
/* fsmi_pool2x: F.avg_pool2d(x, 3, stride=2, padding=1) (count_include_pad) on (B,C,H,W) ->
 *   (B,C,(H-1)/2+1,(W-1)/2+1): pool2x, core/update.py:72-73. */
int fsmi_pool2x(const float* x, float* out, int B, int C, int H, int W, void* stream);

/* ---- disparity transformer of the hourglass ---------
 * fsmi_dt_patch_embed: conv_patch = depthwise Conv3d(C, C, 4, stride 4) + eval
 *   BatchNorm3d (core/foundation_stereo.py:85-88) with bias and BN folded into
 *   per-channel scale / shift; x (B,C,D,H,W) -> out (B,C,D/4,H/4,W/4); w (C,4,4,4).
 * fsmi_disparity_transformer: CostVolumeDisparityAttention.forward
 *   (core/submodule.py:506-528): tokens = the L disparities of each (b,h,w),
 *   x + pe[:L], then nlayers post-norm encoder layers (core/submodule.py:233-257;
 *   attention = FlashMultiheadAttention, :198-229, non-causal, scale 1/sqrt(C/nheads),
 *   FFN with exact GELU, LayerNorm eps).  x, out (B,C,L,HW) NCDHW; pe (L,C);
 *   params = nlayers x fsmi_dt_layer_floats() floats, each layer
 *   [Wq bq Wk bk Wv bv Wo bo ln1.w ln1.b W1 b1 W2 b2 ln2.w ln2.b] (Linear weights
 *   (out,in) row-major).  Built for C=28, 4 heads, FFN 28, L <= 64.
 * fsmi_upsample4_add: vol (B,C,4D,4H,4W) += F.interpolate(t, scale_factor=4,
 *   mode="trilinear", align_corners=False) of t (B,C,D,H,W)
 *   (core/foundation_stereo.py:119-120). */
int fsmi_dt_layer_floats(void);
int fsmi_dt_patch_embed(const float* x, const float* w, const float* scale, const float* shift, float* out,
                        int B, int C, int D, int H, int W, void* stream);
int fsmi_disparity_transformer(const float* x, float* out, const float* params, const float* pe, int B, int C,
                               int L, int HW, int nheads, int ffdim, int nlayers, float eps, void* stream);
int fsmi_upsample4_add(const float* t, float* vol, int B, int C, int D, int H, int W, void* stream);

/* ---- backbone: DepthAnythingV2 ViT + DPT, EdgeNeXt-S, Feature fusion --------
 * replaces Feature / DepthAnythingFeature (core/extractor.py:286-369), the DINOv2 ViT
 * (dinov2/dinov2/models/vision_transformer.py, layers/{attention,block,patch_embed}.py), the DPT head
 * (depth_anything/dpt.py:24-190, depth_anything/blocks.py) and timm's edgenext_small (core/extractor.py:327).
 * The ViT runs on the channel-major token layout (B, C, Tp): token t of channel c at c*Tp + t, the N patch
 * tokens first, the class token at N, zero padding up to Tp; every Linear is then a 1x1 conv of
 * fsmi_conv2d_halo_x3 over a (Tp/32) x 32 "image".
 * fsmi_channel_layernorm: nn.LayerNorm over channels per token (eps), x (B,C,Tx) -> out (B,C,To), tokens
 *   [0, n) (n <= Tx, To); w / b (C) or NULL.  Also LayerNorm2d / channels-last LayerNorm of NCHW maps
 *   (Tx = To = n = H*W).
 * fsmi_vit_attention: softmax(q k^T * scale) v per head (layers/attention.py:69-79): qkv (B, 3*heads*64, Tp)
 *   = [q; k; v] channel-major, out (B, heads*64, Tp); keys >= T masked; head_dim 64; Tp % 64 == 0.
 *   Split-precision MFMA (3 fp16 products per MAC), fp32 softmax.  ws: fsmi_vit_attention_ws_floats(B, heads,
 *   T, Tp) floats (0: NULL allowed) for the key-range partials when the keys are split over several blocks.
 * fsmi_space_to_depth: out[b, (c*k+ky)*k+kx, y, x] = x[b, c, y*k+ky, x*k+kx] (B,C,H,W) -> (B,C*k*k,H/k,W/k):
 *   the im2col of a conv with stride == kernel (patch embed k14, EdgeNeXt stem k4 / downsample k2).
 * fsmi_depth_to_space: out[b, c, y*k+ky, x*k+kx] = x[b, (ky*k+kx)*C + c, y, x]: a ConvTranspose2d with
 *   stride == kernel (DPT resize_layers[0..1]) after its 1x1-conv form.
 * fsmi_vit_tokens: out[b,c,t] = (emb[b,c,t] for t < N | cls[c] for t == N | 0) + pos[c,t] (pos (C,Tp), zero
 *   past N): prepare_tokens_with_masks (vision_transformer.py:214-233) in the layout above.
 * fsmi_resize_bicubic: F.interpolate(mode="bicubic", align_corners=False), A = -0.75, border-clamped taps
 *   (core/extractor.py:352).
 * fsmi_instance_norm: out = act2(act1(InstanceNorm(x)) + res) per plane (planes = B*C, biased variance, no
 *   affine), res may be NULL; act 0 none, 1 ReLU, 6 LeakyReLU(0.01) (core/submodule.py:320-385,
 *   core/extractor.py:20-80 with norm 'instance').
 * fsmi_elementwise: op 0 a+b, 1 relu(a), 2 relu(a+b), 3 a*b; b indexed modulo bper when bper > 0.
 * fsmi_xca: EdgeNeXt cross-covariance attention core (timm CrossCovarianceAttn): qkv (B,3C,N) channel-major,
 *   temperature (heads), ws (fsmi_xca_workspace_floats(B, C, heads) floats: the softmaxed maps, then the
 *   per-split Gram partials), out (B,C,N); C/heads <= 40.
 * fsmi_dwconv2d_ex: fsmi_dwconv2d on channel slices (x / add / out planes at (b*ctot + c)*H*W), KS in
 *   {3,5,7,9}, with add (or NULL) summed into the input first. */
int fsmi_channel_layernorm(const float* x, float* out, const float* w, const float* b, int B, int C, int Tx, int To,
                           int n, float eps, void* stream);
int fsmi_vit_attention(const float* qkv, float* out, int B, int heads, int head_dim, int T, int Tp, float scale,
                       float* ws, long long ws_floats, void* stream);
long long fsmi_vit_attention_ws_floats(int B, int heads, int T, int Tp);
int fsmi_space_to_depth(const float* x, float* out, int B, int C, int H, int W, int k, void* stream);
int fsmi_depth_to_space(const float* x, float* out, int B, int C, int H, int W, int k, void* stream);
int fsmi_vit_tokens(const float* emb, const float* cls, const float* pos, float* out, int B, int C, int N, int Tp,
                    void* stream);
int fsmi_resize_bicubic(const float* x, float* out, int B, int C, int Hi, int Wi, int Ho, int Wo, void* stream);
int fsmi_instance_norm(const float* x, const float* res, float* out, int planes, int HW, float eps, int act1, int act2,
                       void* stream);
int fsmi_elementwise(const float* a, const float* b, float* out, long long n, long long bper, int op, void* stream);
int fsmi_xca(const float* qkv, const float* temperature, float* ws, float* out, int B, int C, int heads, int N,
             void* stream);
long long fsmi_xca_workspace_floats(int B, int C, int heads);
int fsmi_dwconv2d_ex(const float* x, int x_ctot, const float* add, int add_ctot, const float* w, const float* bias,
                     float* out, int out_ctot, int B, int C, int KS, int H, int W, void* stream);

/* ---- after the forward: depth, XYZ map and cloud denoising ---------------
 * The three entry points below take, next to fp32 tensors, a uint8 mask and int64 keys / indices
 * (the one exception to the all-fp32 convention above).
 *
 * Disparity to metric depth and an XYZ map; replaces scripts/run_demo.py:173-251 and
 * depth2xyzmap, Utils.py:56-75.  disp: (B,H,W); xyz: (B,H,W,3); depth: (B,H,W); valid: (B,H,W)
 * uint8.  disp, xyz and depth must be 16-byte aligned, valid 4-byte aligned; B*H*W < 2^31.  One
 * camera serves the whole batch.  For pixel (u = column, v = row):
 *   removed = remove_invisible and u - disp < 0          (run_demo.py:174-178)
 * FSMI_CAMERA_PINHOLE:
 *   depth = fx * baseline / disp, 0 where removed        (run_demo.py:235)
 *   xyz   = ((u-cx) z / fx, (v-cy) z / fy, z), zero where depth < zmin or depth is not finite
 *   valid = not removed, disp finite, 0 < z <= z_far, with z the (zeroed) third component of xyz
 * FSMI_CAMERA_PANORAMA (up/down equirectangular rig, run_demo.py:186-219; fx, fy, cx, cy, zmin and
 * z_far are unused):
 *   lon_up = (2v/H - 1) pi, lat_up = (2u/W - 1) pi/2, lat_down = (2(u-disp)/W - 1) pi/2,
 *   tr = baseline cos(lat_down) / sin(2 pi disp / W), 0 where removed;  depth = tr
 *   xyz = tr (sin lat_up, -cos lat_up cos lon_up, cos lat_up sin lon_up), zero where tr is not finite
 *   valid = not removed, tr finite and positive
 * xyz never holds NaN or inf; depth holds the raw quotient (inf for disp = 0, NaN for NaN). */
#define FSMI_CAMERA_PINHOLE 0
#define FSMI_CAMERA_PANORAMA 1
int fsmi_disp_to_xyz(const float* disp, float* xyz, float* depth, unsigned char* valid, int B, int H, int W,
                     float fx, float fy, float cx, float cy, float baseline, float zmin, float z_far,
                     int remove_invisible, int camera_type, void* stream);
/* Radius outlier removal (scripts/run_demo.py:270-273, Open3D's remove_radius_outlier) on a uniform
 * grid of cell = radius (1 + 2^-20): points closer than radius are at most one cell apart per axis.
 * Step 1, one int64 key per slot.  points: (N,3); valid: (N) uint8 or NULL; keys: (N) int64.
 *   index = clamp(floor(coord / cell), +-(2^20 - 1)) + 2^20 - 1 per axis,
 *   key = ix << 42 | iy << 21 | iz;  INT64_MAX for a slot that is masked out or not finite.
 * The caller sorts the keys ascending (any sort; ties in any order) and gathers the points in that
 * order into rows of 4 floats (x, y, z, unused). */
int fsmi_cloud_cell_keys(const float* points, const unsigned char* valid, long long* keys, int N, float radius,
                         void* stream);
/* Step 2.  sorted_keys: (N) int64 ascending; perm: (N) int64, the slot each sorted row came from;
 * sorted_points4: (N,4), 16-byte aligned; keep: (N) uint8, every slot written.  Each valid point
 * counts the points (itself included) with squared fp32 distance < radius^2 among the 27 cells
 * around its own, stopping once the count exceeds nb_points:  keep[perm[i]] = count > nb_points,
 * 0 for INT64_MAX keys.  N = 0 succeeds and launches nothing (both steps). */
int fsmi_radius_count(const long long* sorted_keys, const long long* perm, const float* sorted_points4,
                      unsigned char* keep, int N, float radius, int nb_points, void* stream);

/* ---- visibility: which disparities belong to pixels the right camera cannot see ----
 * One class per pixel of a rectified LEFT disparity map, from an occlusion z-buffer over the map
 * itself and, with a right-view disparity, the left-right consistency check.  Nothing in the reference
 * pins these definitions (it only drops u - d < 0, scripts/run_demo.py:173-178); they are stated here
 * and restated in numpy by tests/visibility_oracle.py.  One launch after a memset of counts on the same
 * stream; no host synchronisation, no allocation, no float atomics; capturable in a hipGraph.
 *
 * disp: fp32 (B,H,W), 16-byte aligned.  disp_right: NULL, or fp32 (B,H,W), 16-byte aligned, the RIGHT
 * view's disparity on the right image's pixel grid.  classes: uint8 (B,H,W), 4-byte aligned.
 * err: NULL, or fp32 (B,H,W), 16-byte aligned; needs disp_right.  counts: int64 (B, FSMI_VIS_NCLASS),
 * 8-byte aligned, zeroed by the call itself.  1 <= W <= 8192 (FSMI_ERR_ARG beyond: a row's z-buffer and
 * right-view row live in LDS, 8 B per column, so a workgroup stays at or below 64 KiB).
 * occlusion_tol and lr_thresh must not be NaN.
 * For pixel (u = column, v = row) with d = disp[b][v][u], every operation in un-contracted fp32 and in
 * this order; the first matching class wins:
 *   FSMI_VIS_INVALID      d is not finite, or d <= 0
 *   FSMI_VIS_OUT_OF_VIEW  xr = (float)u - d;  xr < 0                        (run_demo.py:174-178)
 *   FSMI_VIS_OCCLUDED     only with occlusion != 0:  c = (int)floorf(xr + 0.5f);  zbuf[c] - d > occlusion_tol,
 *                         zbuf[c] = the largest d over the pixels of the same row that are neither
 *                         INVALID nor OUT_OF_VIEW and have the same c (0 <= xr <= W - 1 puts c in
 *                         [0, W - 1]); the pixel itself is among them, so equal disparities on one
 *                         column occlude nobody
 *   FSMI_VIS_MISMATCH     only with disp_right (dR = its row v of pair b):
 *                           x0 = (int)floorf(xr);  t = xr - (float)x0;  x1 = min(x0 + 1, W - 1)
 *                           r = (t == 0) ? dR[x0] : dR[x0] + t * (dR[x1] - dR[x0])
 *                           e = fabsf(d - r);  MISMATCH iff !(e <= lr_thresh)   (a non-finite r mismatches)
 *   FSMI_VIS_VISIBLE      everything else
 * err[b][v][u] = e for VISIBLE, OCCLUDED and MISMATCH pixels, NaN for INVALID and OUT_OF_VIEW ones.
 * counts[b][k] = the number of pixels of pair b in class k: integer sums, so equal inputs give equal
 * bits in all three outputs.
 * As built: a 256-thread workgroup takes groups of clamp(1024 / W, 1, 8) whole rows of one pair (one
 * group each while B * groups <= 2048 workgroups, several beyond).  Per group it zeroes the rows'
 * z-buffer (uint32) in LDS and copies the right-view rows there, splats with an LDS atomicMax on the
 * bits of d (a positive finite float's bits order like the float, so the maximum is independent of the
 * order of arrival) and classifies; at its end it adds its class counts with one integer atomic per class.  Loads
 * and stores are 16 B / 4 B per lane on the pixels whose flat index is a multiple of 4, whatever the row
 * base; the at most 3 + 3 pixels around them go one by one. */
#define FSMI_VIS_VISIBLE 0
#define FSMI_VIS_INVALID 1
#define FSMI_VIS_OUT_OF_VIEW 2
#define FSMI_VIS_OCCLUDED 3
#define FSMI_VIS_MISMATCH 4
#define FSMI_VIS_NCLASS 5
int fsmi_disp_visibility(const float* disp, const float* disp_right_or_null, unsigned char* classes,
                         float* err_or_null, long long* counts, int B, int H, int W,
                         float occlusion_tol, float lr_thresh, int occlusion, void* stream);

/* ---- photometric consistency: does a disparity explain the two images, without a ground truth ----
 * The right frame warped into the left view by a rectified LEFT disparity, the residual between the
 * left frame and the warp (mean absolute difference, 3x3 SSIM) and, for a few vertical offsets of the
 * right frame, the same absolute difference (the row probe: the offset with the smallest residual is
 * the rig's vertical misalignment).  Nothing in the reference pins these definitions; they are stated
 * here and restated in numpy by tests/photometric_oracle.py.  Two launches (tiles, then one workgroup
 * per pair); no host synchronisation, no allocation, no float atomics; capturable in a hipGraph.
 *
 * disp: fp32 (B,H,W) with batch and row strides in elements, innermost stride 1, 4-byte aligned.
 * left, right: both in image_format, C = 1 or 3 channels, values are grey levels 0..255:
 *   FSMI_IMAGE_F32_PLANAR  fp32 (B,C,H,W) with batch, channel and row strides in elements, innermost
 *                          stride 1, 4-byte aligned (a view of a padded batch goes in as it is)
 *   FSMI_IMAGE_U8_HWC      contiguous uint8 (B,H,W,C); the six image strides are ignored
 * Row strides must be at least W and no stride negative.  mask: NULL, or contiguous uint8 (B,H,W).
 * warped: NULL, or fp32 (B,C,H,W); l1, dssim: NULL, or fp32 (B,H,W); all contiguous and 16-byte aligned
 * (FSMI_ERR_ARG otherwise).  A NULL map costs no store.  row_offsets: n_offsets <= FSMI_PHOTO_MAX_OFFSETS
 * finite fp32 values in HOST memory, read before the call returns.  0 <= alpha <= 1.  ssim != 0 computes
 * the SSIM columns (and the one-pixel halo they need); ssim == 0 leaves them 0 and refuses a dssim map.
 * 1 <= B <= 65535, H * W <= 2^31 - 1; there is no cap on W (nothing is staged by whole rows).
 *
 * Every per-pixel operation is un-contracted fp32 in the order written, divisions IEEE.  For pixel
 * (u = column, v = row) with d = disp[b][v][u], L = left, R = right (as fp32 grey levels):
 *   INVALID      d is not finite, or d <= 0
 *   OUT OF VIEW  otherwise, xr = (float)u - d;  xr < 0
 *   SAMPLED      otherwise;   SCORED = SAMPLED and (mask == NULL or mask[b][v][u] != 0)
 * The sample of channel c at row offset dy (the main path is dy = 0, where w = h(v)):
 *   x0 = floorf(xr), t = xr - x0, x1 = min(x0 + 1, W - 1)
 *   h(y) = (t == 0) ? R[c][y][x0] : R[c][y][x0] + t * (R[c][y][x1] - R[c][y][x0])
 *   yr = (float)v + dy; the pixel counts for that offset only if 0 <= yr <= (float)(H - 1);
 *   y0 = floorf(yr), ty = yr - y0, y1 = min(y0 + 1, H - 1);  w = (ty == 0) ? h(y0) : h(y0) + ty * (h(y1) - h(y0))
 *   l1(dy) = |L[0] - w[0]|                                         C = 1
 *          = ((|L[0] - w[0]| + |L[1] - w[1]|) + |L[2] - w[2]|) / 3.0f    C = 3
 * warped[b][c][v][u] = w at dy = 0 for SAMPLED pixels, 0 elsewhere.  l1[b][v][u] = l1(0) for SCORED pixels,
 * +inf elsewhere.
 * SSIM is defined for a SCORED pixel with 1 <= u <= W - 2, 1 <= v <= H - 2 whose nine 3x3 neighbours are
 * all SAMPLED (masked in or not).  Per channel, x_k = L and y_k = warped at the taps k = 0..8 in row-major
 * order ((v-1,u-1), (v-1,u), ... (v+1,u+1)), every sum starting from its k = 0 term and adding k = 1..8 in
 * order:
 *   mx = (sum x_k) / 9.0f,  my likewise
 *   vx = (sum (x_k - mx) * (x_k - mx)) / 9.0f,  vy likewise,  cxy = (sum (x_k - mx) * (y_k - my)) / 9.0f
 *   num = ((2.0f * mx) * my + 6.5025f) * (2.0f * cxy + 58.5225f)
 *   den = ((mx * mx + my * my) + 6.5025f) * ((vx + vy) + 58.5225f)
 *   ds  = (1.0f - num / den) * 0.5f;  if !(ds >= 0) ds = 0;  if (ds > 1) ds = 1
 * dssim[b][v][u] = ds for C = 1, ((ds[0] + ds[1]) + ds[2]) / 3.0f for C = 3; +inf where SSIM is undefined.
 * (The variance is the centred two-pass form: E[x^2] - E[x]^2 cancels at 255^2.)
 *
 * sums, table: fp64 (B, FSMI_PHOTO_NFIXED + 2 * n_offsets), 8-byte aligned.  Per-pixel values are widened
 * to fp64 before they are added (l1 * l1 is formed in fp64); counts are exact doubles.
 *   sums[b]  = [n_scored, n_ssim, n_invalid, n_out_of_view, sum l1, sum l1^2 (both over SCORED pixels),
 *               sum dssim, sum l1 (both over SSIM pixels), then per offset r: n_r, sum l1(dy_r)]
 *              n_r counts the SCORED pixels whose yr is in range
 *   table[b] = [n_scored, n_ssim, n_invalid, n_out_of_view, sums[4] / n_scored, sqrt(sums[5] / n_scored),
 *               sums[6] / n_ssim, (alpha * sums[6] + ((1 - alpha) * sums[7]) / 255) / n_ssim,
 *               then per offset r: n_r, sum / n_r]       in fp64; a mean over zero pixels is 0
 * Column 7, "photometric", is the mean over the SSIM pixels of alpha * dssim + (1 - alpha) * l1 / 255.
 * workspace: fsmi_photo_consistency_ws_bytes(B, H, W, n_offsets) bytes (0 for arguments the call would
 * refuse), 8-byte aligned; every row is written, none is read before it is.  The order of every addition
 * is a function of (B, H, W, n_offsets) alone: a workgroup's 256 lanes reduce through a fixed shuffle
 * tree and LDS into one stored row per tile, the second launch adds a pair's rows in index order.
 * Equal inputs give equal bits.
 * As built: a 256-thread workgroup takes a 64 x 12 tile of one pair.  It reads disp and left once for
 * the tile and, with SSIM, a one-pixel halo, 16 B per lane (4 B for uint8 C = 1, 12 B for C = 3) on
 * the quads of columns 4k .. 4k+3 whose address is 16-byte (uint8: 4-byte) aligned, one by one
 * elsewhere; gathers the right taps from global memory (neighbouring pixels' taps share cache lines);
 * keeps left, warped, xr and the class in LDS, so each warped value is computed once and the nine
 * windows that hold it read it from LDS; then scores the tile's own pixels and stores the maps
 * 16 B per lane under the same rule.  The row probe re-gathers the right taps per offset in the same
 * launch; the left image and disp are not read again. */
#define FSMI_IMAGE_F32_PLANAR 0
#define FSMI_IMAGE_U8_HWC 1
#define FSMI_PHOTO_NFIXED 8
#define FSMI_PHOTO_MAX_OFFSETS 8
int fsmi_photo_consistency(const float* disp, const void* left, const void* right, const unsigned char* mask_or_null,
                           float* warped_or_null, float* l1_or_null, float* dssim_or_null, double* table, double* sums,
                           double* workspace, int B, int C, int H, int W, int image_format, long long disp_batch_stride,
                           long long disp_row_stride, long long left_batch_stride, long long left_channel_stride,
                           long long left_row_stride, long long right_batch_stride, long long right_channel_stride,
                           long long right_row_stride, const float* row_offsets, int n_offsets, double alpha, int ssim,
                           void* stream);
size_t fsmi_photo_consistency_ws_bytes(int B, int H, int W, int n_offsets);

/* ---- confidence: how sure the cost volume was of a disparity -------------
 * The classifier's logits are a distribution over the D = max_disp / 4 bins of every quarter-resolution
 * pixel; soft-argmin keeps its mean.  This reads the rest: four per-pixel confidence channels on the
 * full-resolution grid of the disparity they judge.  Nothing in the reference pins these definitions;
 * they are stated here and restated in numpy by tests/confidence_oracle.py.  One launch; no host
 * synchronisation, no allocation, no atomics; capturable in a hipGraph.
 *
 * logits: fp32 (B,D,h,w), contiguous, the classifier output before the softmax.  up in 1..8; the maps
 * are (B,H,W) with H = h * up, W = w * up.  disp: NULL ("self" mode), or fp32 (B,H,W).  mass, spread, peak,
 * entropy: NULL, or fp32 (B,H,W); at least one is not NULL, a NULL map costs no store.  Every pointer is
 * 4-byte aligned; disp and the maps are accessed 16 B at a time where up == 4 and all of them are
 * 16-byte aligned, one float at a time otherwise.  1 <= D <= FSMI_CONF_MAX_D; radius is finite and >= 0; H * W <= 2^31 - 1
 * (FSMI_ERR_ARG otherwise).
 *
 * Output pixel (y, x) of pair b reads the column x_0 .. x_{D-1} = logits[b][.][y / up][x / up] (integer
 * division: the nearest column, the centre tap of the convex upsampling).  Every operation is
 * un-contracted fp32 in the order written, every sum starts at 0 and adds d = 0, 1, .. D-1 in order,
 * divisions and square roots IEEE, expf / logf the device library's:
 *   m   = max_d x_d                                  t_d = x_d - m          e_d = expf(t_d)
 *   s   = sum e_d                                    (p_d = e_d / s is the distribution)
 *   mu  = (sum e_d * (float)d) / s                   the column's expectation, in bins
 *   var = (sum e_d * (((float)d - mu) * ((float)d - mu))) / s
 *   set = sum (e_d != 0 ? e_d * t_d : 0)             Hn = logf(s) - set / s        (the entropy, nats)
 *   q   = disp[b][y][x] * disp_scale                 one multiply: the query, in bins (self mode: q = mu)
 *   peak    = 1.0f / s                               the largest probability
 *   entropy = D == 1 ? 1 : min(max(1.0f - Hn / logf((float)D), 0), 1)     (logf((float)D) on the host)
 *   mass    = min((sum e_d * w_d) / s, 1),  w_d = min(max((radius + 1.0f) - fabsf((float)d - q), 0), 1)
 *             a trapezoid: full weight within radius bins of q, falling linearly to 0 one bin further,
 *             so it is continuous in q; for integer q and radius it is the probability within +-radius
 *             bins.  radius + 1.0f is formed once, on the host.
 *   spread  = sqrtf(var + (mu - q) * (mu - q))       sqrt(sum p_d (d - q)^2): RMS distance from q, bins
 * peak, entropy and mass are in [0, 1] (the two clamps only take back a last-bit excess).
 * A column that holds a NaN or a +inf logit, or only -inf logits, gives NaN in all four maps at its
 * up x up pixels; -inf logits otherwise count as probability 0.  A non-finite q gives NaN in mass and
 * spread only.
 * As built: one lane per column, lanes over w (every plane load coalesced), 64-thread workgroups (at
 * 640x480, B = 1 there are 19 200 columns for 256 CUs).  The column statistics are computed once per
 * column.  D <= 128: the column is loaded from HBM once into registers (tiers of 16 / 64 / 128), e_d
 * replaces x_d there, one expf per element.  Above: three streaming passes, the second and third from
 * L1 / L2, two expf per element.  Per output pixel only mass needs the column again: the
 * min(ceil(2 (radius + 1)) + 3, D) bins from floorf(q - (radius + 1)) on that exist are re-read, four bins of each pixel of an output row at a time so
 * that the loads, L1 / L2 hits, are independent.  (The fp32 difference under the floorf errs by far less
 * than a bin and the window carries a spare bin at either end, so the bins left out are ones whose fp32
 * weight is 0; tests/confidence_oracle.py sums all D bins and the device is held to the tolerances there,
 * not to its bits.)  A lane stores up consecutive floats per output row,
 * 16 B at a time (and loads disp so) where up == 4 and the bases are 16-byte aligned. */
#define FSMI_CONF_MAX_D 1024
#define FSMI_CONF_MAX_UP 8
int fsmi_disp_confidence(const float* logits, int B, int D, int h, int w, const float* disp_or_null, int up,
                         float disp_scale, float radius, float* mass, float* spread, float* peak, float* entropy,
                         void* stream);

/* ---- risk-coverage: grade a confidence by the error of the pixels it would drop first ----
 * The histogram behind the sparsification curve: pixels binned by confidence, per bin the pixel count
 * and the sum of |pred - gt|.  Integers throughout, so the result does not depend on the order of the
 * additions (integer atomics in LDS and global memory) and tests/confidence_oracle.py reproduces it bit
 * for bit.  One launch after a memset of the three outputs on the same stream; no host synchronisation.
 *
 * conf: NULL (the oracle ranking: bin by the error itself), or fp32 (B,H,W).  pred, gt: fp32 (B,H,W).
 * mask: NULL, or uint8 (B,H,W).  All contiguous; fp32 maps 4-byte aligned.  count, err_q20: int64
 * (B,nbins); dropped: int64 (B); 8-byte aligned, zeroed by the call itself.  2 <= nbins <=
 * FSMI_RISK_MAX_BINS, err_bin_scale finite and > 0, H * W <= 2^31 - 1 (FSMI_ERR_ARG otherwise).
 * Per pixel, un-contracted fp32:
 *   valid   mask != NULL ? mask != 0 : (gt > 0 and gt finite)         (as fsmi_disp_metrics)
 *   e     = fabsf(pred - gt)
 *   a valid pixel whose pred is not finite, or whose c = conf fails 0 <= c <= 1 (NaN fails, -0.0
 *   passes), adds 1 to dropped[b] and nothing else
 *   bin   = min(nbins - 1, (int)(c * (float)nbins))                                    conf != NULL
 *         = nbins - 1 - k,  v = e * err_bin_scale,  k = v < (float)(nbins - 1) ? (int)v : nbins - 1
 *           (NaN compares false: the worst bin)                                        conf == NULL
 *   count[b][bin] += 1;   err_q20[b][bin] += (long long)(fminf(e, 4096.0f) * 1048576.0f)
 * The product by 2^20 is exact and the truncation a function of the value alone; fminf returns 4096
 * for a NaN e (a non-finite gt under a mask).
 * As built: 256-thread workgroups, each striding over the pixels of one pair with a (count u32, sum
 * u64) histogram in LDS, flushed once with one 64-bit global atomic per non-empty bin. */
#define FSMI_RISK_MAX_BINS 1024
int fsmi_risk_coverage(const float* conf_or_null, const float* pred, const float* gt,
                       const unsigned char* mask_or_null, int B, int H, int W, int nbins, float err_bin_scale,
                       long long* count, long long* err_q20, long long* dropped, void* stream);

/* ---- around the forward: frame ingest and the disparity picture -----------
 * uint8 frames in, uint8 pictures out (with the cloud section, the exceptions to the all-fp32
 * convention).  Nothing below synchronises the host; all of it can be captured in a hipGraph.
 *
 * Two camera frames to model input; replaces scripts/run_demo.py:131-159.  left, right: uint8
 * (B,H,W,C), C = 1 (gray, replicated to three channels, :134-138), 3, or 4 (alpha dropped, :139-141).
 * out: fp32 (B,2,3,Hp,Wp), [left, right] per pair, 16-byte aligned: the batch layout of
 * dist.ShardedStereo / bench.py.  image_u8: NULL, or uint8 (B,Hs,Ws,3), the resized unpadded left
 * frame (the reference's img0_ori).  One launch serves both frames of every pair.
 * The HOST computes and passes in:
 *   Hs, Ws   the resized size, round-half-even of H * scale and W * scale (cv2.resize(fx, fy,
 *            dsize=None)'s cvRound; Python's round()); 0 < scale <= 1, and scale == 1 needs (Hs,Ws) == (H,W)
 *   pads     InputPadder(mode='sintel', divis_by) of (Hs, Ws), core/utils/utils.py:26-29,35:
 *            pad = (((n / d) + 1) d - n) % d, left / top get pad / 2, right / bottom the rest;
 *            Hp = Hs + pad_top + pad_bottom and Wp likewise must be multiples of divis_by, Wp of 4 too
 * The kernel computes, for padded pixel (yp, xp), the resized pixel
 *   (ys, xs) = (clamp(yp - pad_top, 0, Hs-1), clamp(xp - pad_left, 0, Ws-1))           (replicate padding)
 * and its value: scale == 1, the source byte (no arithmetic); otherwise cv2.INTER_LINEAR as it
 * shrinks, half-pixel centres and no antialiasing:
 *   sx = (xs + 0.5) / scale - 0.5 (fp64), x0 = floor(sx), wx = fp32(sx - x0), taps x0 and x0 + 1
 *   clamped to [0, W-1]; rows likewise; in un-contracted fp32  top = a + (b - a) wx,  bot likewise,
 *   v = top + (bot - top) wy;  result = clamp(floor(v + 0.5), 0, 255)  (half rounds up, as cv2's
 *   fixed-point (sum + half) >> shift does on exact ties; an integer, as the reference resizes uint8)
 * ImageNet normalisation is not applied here: it stays inside the forward, as in the reference. */
int fsmi_frames_ingest(const unsigned char* left, const unsigned char* right, float* out, unsigned char* image_u8,
                       int B, int H, int W, int C, double scale, int Hs, int Ws, int pad_left, int pad_right,
                       int pad_top, int pad_bottom, int divis_by, void* stream);
/* The picture of a disparity map; replaces vis_disparity, Utils.py:108-133 (run_demo.py:168-170).
 * A pixel is VALID when it is not NaN and not >= invalid_thres (Utils.py:115; NaN is this library's
 * definition: the reference's min() would return NaN and its uint8 cast is undefined).
 * Step 1.  disp: (B,H,W), 16-byte aligned; minmax: (B,2) fp32.  The function itself sets minmax to
 * (+inf, -inf) on the stream, then writes each image's min and max over its valid pixels
 * (Utils.py:120-123); an image without a valid pixel keeps (+inf, -inf).  Exact and independent of
 * the order in which blocks finish. */
int fsmi_disp_minmax(const float* disp, float* minmax, int B, int H, int W, float invalid_thres, void* stream);
/* Step 2.  minmax: (B,2) from step 1, or filled by the caller from explicit min_val / max_val;
 * lut: uint8 (256,3) RGB on the device; image: NULL, or uint8 (B,H,W,3); out: uint8 (B,H,Wout,3),
 * 4-byte aligned, Wout = 2W with an image (columns [0,W) the image, [W,2W) the colours: the demo's
 * np.concatenate([img0_ori, vis], axis=1), run_demo.py:169), else W.  Per valid pixel, in fp32 with
 * IEEE division and no contraction (Utils.py:126-130 with the table indexed directly):
 *   t = clip((d - mn) / (mx - mn), 0, 1) * 255;  rgb = lut[(unsigned char) t]      (truncation)
 * mx == mn maps every valid pixel to lut[0] (the reference divides by zero).  Invalid pixels are
 * (0,0,0) (:131-132), so an image without a valid pixel is all zeros (:116-119). */
int fsmi_disp_colorize(const float* disp, const float* minmax, const unsigned char* lut, const unsigned char* image,
                       unsigned char* out, int B, int H, int W, float invalid_thres, void* stream);

/* ---- scoring a disparity map against a ground truth ----------------------
 * Per-pair EPE, RMSE, bad-pixel rates, KITTI's D1 and the prediction's own statistics; replaces
 * compute_stereo_metrics (train/utils.py:88-141, train/losses.py:342-376) and monitoring_stereo
 * (train/losses.py:326-339), which gather through a boolean mask and read 4 + K scalars back per pair.
 * Nothing below synchronises the host or allocates; all of it can be captured in a hipGraph.  Sums
 * are fp64 and no float atomic is used: every addition's order is fixed by (H*W, the block count)
 * alone, and the block count by H*W alone, so equal inputs give equal bits on every device.
 *
 * pred: fp32 (B,H,W), 16-byte aligned.  The ground truth is exactly one of
 *   gt      fp32 (B,H,W), 16-byte aligned, or
 *   gt_u8   uint8 (B,H,W,3), 4-byte aligned, the reference's encoding (depth_uint8_decoding,
 *           Utils.py:137-140):  n = r * 65025 + g * 255 + b  (int32, at most 16 605 816),
 *           gt = (float)((double)n / gt_scale), gt_scale > 0
 * mask: NULL, or uint8 (B,H,W), 4-byte aligned.  A pixel is VALID where mask != 0 when a mask is
 * given (the mask alone decides, as in the reference); otherwise where gt > 0 && gt < +inf (the
 * dataloader's rule, train/dataloader.py:142-148, with NaN and inf ground truth invalid).
 * thresholds: K <= FSMI_METRICS_MAX_THRESHOLDS fp32 values in HOST memory, read before the call returns.
 * Per valid pixel, in un-contracted fp32 as torch evaluates it on fp32 tensors:
 *   e = fabsf(pred - gt);   bad[k] counts e > thresholds[k];   d1 counts e > 3 && e > 0.05f * fabsf(gt)
 *   (KITTI's D1-all); e and e * e are widened to fp64 before they are added.
 * NaN and inf propagate as in torch: a NaN prediction under a valid pixel makes the sums NaN, is "not
 * bad" in every rate (NaN > t is false) and is counted in n_nonfinite.
 * partials: workspace, (B, fsmi_disp_metrics_blocks of (H,W), FSMI_METRICS_NACC) fp64; every row is
 * written, none is read before it is.  sums, table: (B, FSMI_METRICS_NACC) fp64.
 *   sums[b]  = [n_valid, sum e, sum e^2, n_d1, n_nonfinite, sum (x - x0), sum (x - x0)^2, min x, max x,
 *               n_bad[0..7]]   x = pred over ALL pixels of the pair, x0 = pred[b,0,0] (the shift keeps
 *               the one-pass variance well conditioned); counts are exact doubles; min and max
 *               propagate NaN; unused n_bad slots are 0.  The sums of several calls add.
 *   table[b] = [n_valid, epe, rmse, d1_all, n_nonfinite, pred_mean, pred_std, pred_min, pred_max,
 *               bad[0..7]]   epe = sum e / n, rmse = sqrt(sum e^2 / n), rates = count / n, all fp64;
 *               n_valid == 0 gives epe = rmse = d1_all = bad[k] = 0 (train/utils.py:122-123);
 *               pred_std is the unbiased one (torch's default), NaN for a one-pixel map; a sum of
 *               squared deviations that rounds below 0 counts as 0.
 * error: NULL, or fp32 (B,H,W), 16-byte aligned: e on valid pixels, +inf on invalid ones (with
 * fsmi_disp_colorize at min 0, max tau: an error picture whose invalid pixels are black). */
#define FSMI_METRICS_NACC 17
#define FSMI_METRICS_MAX_THRESHOLDS 8
/* Blocks per pair of the streaming pass: a function of H * W only, never of the device; >= 1. */
int fsmi_disp_metrics_blocks(int H, int W);
int fsmi_disp_metrics(const float* pred, const float* gt, const unsigned char* gt_u8, const unsigned char* mask,
                      const float* thresholds, int K, double gt_scale, double* partials, double* sums, double* table,
                      float* error, int B, int H, int W, void* stream);
/* The ground-truth map itself: gt_u8 uint8 (B,H,W,3), 4-byte aligned -> out fp32 (B,H,W), 16-byte
 * aligned, the arithmetic above (bit-equal to float32 of the reference's float64 decode). */
int fsmi_gt_decode(const unsigned char* gt_u8, float* out, int B, int H, int W, double gt_scale, void* stream);

/* ---- scoring a sequence of disparity maps: every refinement iteration in one pass ----
 * R <= FSMI_SEQ_MAX_ROWS prediction maps ("rows") of one batch against one ground truth: per (pair,
 * row) EPE, RMSE, smooth-L1, bad-pixel rates and D1, and per pair the weighted sequence loss; replaces
 * foundation_stereo_loss and the single-map losses beside it (train/losses.py:20-187, :379-498), which
 * gather through a boolean mask once per map, resize with F.interpolate and read about 7 scalars back
 * per map.  Like the stage above: no host synchronisation, no allocation, no float atomics, capturable.
 *
 * Row r is an fp32 map (B, hs[r], ws[r]) given by its base pointer rows[r] (4-byte aligned; device
 * memory), the stride between pairs batch_strides[r] and between lines row_strides[r] (in elements,
 * row_strides[r] >= ws[r]; the element stride is 1): views such as padder.unpad's go in as they are.
 * The nine per-row arrays (rows .. smooth) are R values each in HOST memory, read before the call
 * returns.  gt, gt_u8, mask, thresholds, gt_scale and validity are fsmi_disp_metrics's, except that gt
 * needs 4-byte and gt_u8 / mask 1-byte alignment only.  Per VALID pixel (y, x) and row r, in
 * un-contracted fp32 as torch evaluates it:
 *   1. v = row[y][x] when (hs[r], ws[r]) == (H, W); otherwise the bilinear sample of
 *      F.interpolate(align_corners=False): per axis, with s = (float)in / (float)out rounded once on
 *      the host,  src = max(s * (dst + 0.5f) - 0.5f, 0);  i0 = min((int)src, in - 1);
 *      i1 = min(i0 + 1, in - 1);  l1 = src - i0;  l0 = 1 - l1;  then
 *      v = l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11)
 *   2. v = v * muls[r]
 *   3. max_disps[r] < +inf:  v = v < 0 ? 0 : v;  v = v > max_disps[r] ? max_disps[r] : v  (torch.clamp:
 *      a NaN stays NaN).  max_disps[r] = +inf: no clamp at either end.
 *   4. e = fabsf(v - gt)
 *   5. sl1 = beta == 0 ? e : (e < beta ? (0.5f * (e * e)) / beta : e - 0.5f * beta)   (IEEE division)
 *   bad[k], d1 and nonfinite are counted on e as fsmi_disp_metrics counts them; (double)e,
 *   (double)e * (double)e and (double)sl1 are what is added.
 * partials: workspace, (B, R, fsmi_seq_metrics_blocks of (H,W,R), FSMI_SEQ_NACC) fp64; every row is
 * written, none is read before it is.  sums, table: (B, R, FSMI_SEQ_NACC) fp64; loss: (B) fp64.
 *   sums[b][r]  = [n_valid, sum e, sum e^2, sum sl1, n_d1, n_nonfinite, n_bad[0..7]]   additive over
 *                 pairs and calls; counts are exact doubles; unused n_bad slots are 0
 *   table[b][r] = [n_valid, epe, rmse, smooth_l1, d1_all, n_nonfinite, bad[0..7]]   means and rates over
 *                 n_valid, rmse = sqrt(sum e^2 / n); n_valid == 0 gives zeros (train/losses.py:60)
 *   loss[b]     = sum over r, added in row order in fp64 without contraction, of
 *                 weights[r] * (smooth[r] ? table[b][r].smooth_l1 : table[b][r].epe)
 *                 (row 0 = the initial disparity, smooth, weight 1, and rows 1..K = the iterations with
 *                 weights gamma^(K-k): foundation_stereo_loss's total_loss)
 * Order of the additions: a block adds its pixels lane by lane in index order and reduces by a fixed
 * shuffle tree; the finalize kernel (one block per pair, once per call) adds the blocks' partial rows
 * in index order and finishes with the same tree.  It is fixed by (H*W, the block count) alone, and
 * the block count by (H*W, R) alone: equal inputs give equal bits, run to run and in a graph replay. */
#define FSMI_SEQ_NACC 14
#define FSMI_SEQ_MAX_ROWS 64
/* Partial rows per (pair, prediction row) of the streaming pass: a function of its arguments only; >= 1. */
int fsmi_seq_metrics_blocks(int H, int W, int R);
int fsmi_seq_metrics(const float* const* rows, const long long* batch_strides, const long long* row_strides,
                     const int* hs, const int* ws, const float* muls, const float* max_disps, const double* weights,
                     const unsigned char* smooth, int R, const float* gt, const unsigned char* gt_u8,
                     const unsigned char* mask, const float* thresholds, int K, double gt_scale, float beta,
                     double* partials, double* sums, double* table, double* loss, int B, int H, int W, void* stream);

/* ---- live kernel timing (bench.py roofline) -----------------------------
 * When enabled, every launch of the kernels below is bracketed by a pair of
 * hipEvents recorded on the launch stream (skipped while the stream is being
 * captured).  fsmi_timer_query synchronises those events and returns the
 * summed duration and launch count since the last reset. */
enum {
  FSMI_K_GWC = 0, FSMI_K_CONCAT, FSMI_K_COMB, FSMI_K_PROJ, FSMI_K_CORR, FSMI_K_VOLPYR,
  FSMI_K_LOOKUP, FSMI_K_SAMPLER, FSMI_K_REG, FSMI_K_UPSAMPLE, FSMI_K_GRU_RESET, FSMI_K_GRU_BLEND,
  FSMI_K_CONV3D, FSMI_K_CONV2D, FSMI_K_DWCONV, FSMI_K_RESIZE, FSMI_K_DT, FSMI_K_NORM, FSMI_K_COUNT
};
/* Range guard of the split-precision convs: a block scales its activations by a power of two
 * fixed from its first 32-channel chunk (8 bits of headroom); a later value that would still
 * leave fp16's range sets a host-mapped flag instead of silently becoming inf.  *overflowed =
 * the flag (1 once any conv since the last reset overflowed); reset != 0 clears it.  The flag
 * is written asynchronously: synchronise the streams that ran the convs before reading it. */
int fsmi_range_status(int reset, int* overflowed);
/* Safe range mode: while set, every split-precision 2D conv launched (or captured) afterwards takes
 * a per-chunk block exponent with exact accumulator rescaling (the volumes' mode), which cannot
 * overflow; ~3 % slower.  FoundationStereo.forward switches it on and re-runs a forward whose
 * range flag came back set (the reference has no such mode: its convs are fp32 / fp16 autocast,
 * core/update.py:83-159).  Sticky until cleared. */
int fsmi_set_range_safe(int safe);
/* Fill out[0..n) with NaN on `stream` when the range flag is set (a device-side check, no host
 * synchronisation): FoundationStereo.forward appends it to a CAPTURED forward, so a graph replay
 * whose convs overflowed returns NaN, never a silently wrong disparity. */
int fsmi_range_poison(float* out, long long n, void* stream);
int fsmi_get_range_safe(int* safe);

/* on: 0 off, 1 on (events + kernel clocks outside stream capture), 2 also the kernel clocks of
 * launches captured into a hipGraph (their stamps are rewritten by every replay: a query after the
 * replays reads the last replay's launches -- bench.py's in-step lookup timing), 3 as 2 with every
 * instrumented kernel clocked, not only the geometry kernels (fsmi_timer_dump_captured). */
int fsmi_timer_enable(int on);
int fsmi_timer_reset(void);
int fsmi_timer_query(int kernel, double* total_ms, long long* count);
/* Same launches timed by the kernels themselves (lookup, cost-volume build, all-pairs correlation
 * and its normalisation, volume pyramid): each
 * instrumented launch records its first block start and last wave end (stores acknowledged) in
 * s_memrealtime ticks; returns the summed durations -- execution time without the latency of
 * the event records around the launch. */
int fsmi_timer_query_clock(int kernel, double* total_ms, long long* count);
/* The same over the launches captured into hipGraphs while timing was in mode 2: their stamps hold
 * the last replay of each graph.  Kept across fsmi_timer_reset / fsmi_timer_enable (the graphs keep
 * writing their slots) until fsmi_timer_release_captured, which the caller may call only once every
 * graph captured in mode 2 is destroyed (their slots are then handed out again).  Either query fails
 * (FSMI_ERR_ARG) when a launch of the kernel found the clock arena full (16M stamps; 64M in timer mode 3). */
int fsmi_timer_query_clock_captured(int kernel, double* total_ms, long long* count);
int fsmi_timer_release_captured(void);
/* The replay's timeline: one text line per launch captured in timer mode 2, in capture order,
 * "<kernel id> <stream> <first wave start> <last wave end> <tag>" (s_memrealtime ticks, 100 MHz;
 * 0 0 for a launch no replay has run).  Writes at most size bytes (NUL-terminated); *needed = the
 * full length + 1.  Instrumented: the halo / pointwise conv kernels and their split-K reduce, the
 * EdgeNeXt MLP, depthwise / 1-input convs, pool / resize, and the geometry kernels. */
int fsmi_timer_dump_captured(char* buf, long long size, long long* needed);
/* The number of lines fsmi_timer_dump_captured would print so far (launches captured with clocks),
 * without touching the device: callable while a capture is in progress (positions a cross-stream wait
 * among the captured launches; tools/replay_timeline.py). */
int fsmi_timer_captured_count(long long* n);
/* *id = the id of the hipGraph capture `stream` is part of (hipStreamGetCaptureInfo), -1 when it is not capturing. */
int fsmi_stream_capture_id(void* stream, long long* id);
/* Re-issue the last timed launch of `kernel` (lookup, cost-volume build) `reps` times back to
 * back on its stream between two hipEvents; *avg_ms = span / reps.  The kernels are pure
 * functions of their inputs, so the replays rewrite identical outputs.
 * Lifetime contract: the replay reuses the raw device pointers of the recorded launch, so the
 * CALLER must keep every input and output buffer of that launch allocated until the replay has
 * finished (ops.py holds references to the last timed launch's tensors until the next
 * fsmi_timer_reset / fsmi_timer_enable, which also drop the recorded launch). */
int fsmi_timer_replay(int kernel, int reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* FSMI_H_ */
