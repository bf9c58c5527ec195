/*
 * semstereo_hip.h -- C ABI of libsemstereo_hip.so: the MI355X (gfx950) kernels for the
 * SemStereo cost-volume + 3-D aggregation hot path.
 *
 * The reference (chenchen235/SemStereo) is pure Python: its "operator interface" for this
 * path is a set of module-level callables in models/submodule.py that models/SemStereo.py
 * star-imports and calls by bare name.  Each entry point below is the
 * device-side replacement of one of those callables (or of one nn.Module.forward on the
 * path); the Python wrappers in semstereo_amd/ops.py keep the reference names and positional
 * signatures and call these through ctypes.
 *
 * Conventions
 *  - all tensors are fp32, contiguous, in the reference's layouts: NCHW feature maps,
 *    NCDHW volumes;
 *  - pointers are BORROWED device pointers (owned by the caller's allocator); outputs are
 *    fully written by the kernels (no pre-zeroing needed) unless stated;
 *  - `stream` is a hipStream_t (NULL = the null stream); launches are asynchronous;
 *  - re-entrant, no global mutable state, current device of the calling thread;
 *  - return value: SS_OK (0) or a negative ss_status; nothing throws across the ABI.
 *  - parameters are int, long long, float, double, ss_stream_t or pointers: semstereo_amd/_lib.py binds from these declarations and refuses any other type.
 */
#ifndef SEMSTEREO_HIP_H
#define SEMSTEREO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ss_stream_t; /* hipStream_t */

enum ss_status {
    SS_OK = 0,
    SS_ERR_INVALID = -1,     /* null pointer, non-positive size, C % groups != 0 ... */
    SS_ERR_UNSUPPORTED = -2, /* shape outside what the kernels are built for */
    SS_ERR_LAUNCH = -3       /* hipGetLastError() != hipSuccess after the launch */
};

/* ABI version (19 since round 6 (13-18 earlier in it); 12 since round 5; ss_abi_version() is authoritative and semstereo_amd/_lib.py checks it at load): bumped on any
 * signature change or new entry point the Python binding requires. */
int ss_abi_version(void);
/* The library's tuning switches (SS_CONV_TILE, SS_GWC_STREAM, SS_WARP_STREAM, SS_WARP_VEC, SS_DECONV_SPLIT, ...; A/B
 * measurement aids) are read from the environment ONCE per process; call this after changing
 * one of them.  No reference counterpart (the reference has no tuning surface). */
int ss_reload_tuning(void);
/* "The chip is shared": how many pairs are in flight on the device at once (PairPipeline's lanes), process-wide, default 1.  Read at
 * launch time by the FILL heuristics of the 3x3x3 conv launchers only -- which output tile a stride-1 layer gets, which form a
 * stride-2 layer -- whose thresholds count workgroups: a launch that is one of N in flight need not cover the chip by itself and gets
 * the larger, cheaper-per-MFMA tile.  Nothing that fixes the summation order reads it (chunk-blocked accumulation stays a property
 * of the LAYER's own per-pair size), and every tile candidate gives the same bits, so the value -- and a race on it between threads
 * -- changes speed only, never results.  Clamped to [1, 64].  ss_set_fill_hint returns the PREVIOUS value (to restore it);
 * ss_get_fill_hint returns the value the launchers use now, i.e. the environment override SS_FILL_HINT (>= 1, read with the other
 * tuning switches) if that is set.  No reference counterpart. */
int ss_set_fill_hint(int pairs_in_flight);
int ss_get_fill_hint(void);
/* Static, human-readable text for an ss_status. */
const char* ss_status_string(int status);
/* hipGetErrorString of the last SS_ERR_LAUNCH on this thread ("" if none). */
const char* ss_last_hip_error(void);

/* ---- disparity ranges -------------------------------------------------------------------
 * Every volume / regression entry point takes (dmin, ndisp): plane p of a volume holds disparity dmin + p.
 *   signed op set    models/submodule.py   (models/SemStereo.py):      dmin = -maxdisp, ndisp = 2 * maxdisp
 *   unsigned op set  models/submodule_.py  (what models/SemStereo_WHU.py:279,305 is written for): dmin = 0, ndisp = maxdisp */

/* ---- group-wise correlation ----------------------------------------------------------
 * groupwise_correlation(fea1, fea2, num_groups)       models/submodule.py:190-196
 * groupwise_correlation_norm(...)                     models/submodule.py:213-221
 * out[b,g,y,x] = mean_c f1[b,g*Cg+c,y,x] * f2[b,g*Cg+c,y,x]; with normalize != 0 each group
 * vector is first divided by (its L2 norm over the Cg channels + 1e-5).  [B,C,H,W]^2 -> [B,G,H,W] */
int ss_groupwise_correlation_fwd(const float* fea1, const float* fea2, float* out,
                                 int B, int C, int H, int W, int groups, int normalize,
                                 ss_stream_t stream);

/* build_gwc_volume(ref, tgt, maxdisp, num_groups)      models/submodule.py:198-211   (unsigned: models/submodule_.py:188-198)
 * build_gwc_volume_norm(...)                           models/submodule.py:224-238 (live: SemStereo.py:273; unsigned :211-221)
 * out[b,g,p,y,x] = corr(ref[...,x], tgt[...,x-(dmin+p)]) for p in [0, ndisp), 0 where
 * the partner column leaves the image.  [B,C,H,W]^2 -> [B,G,ndisp,H,W] */
int ss_gwc_volume_fwd(const float* ref, const float* tgt, float* out,
                      int B, int C, int H, int W, int dmin, int ndisp, int groups, int normalize,
                      ss_stream_t stream);
/* models/SemStereo.py:273-276 in one launch: build_gwc_volume[_norm] -> `patch` (depthwise Conv3d, kernel (1,3,3),
 * padding (0,1,1), no bias; patch_w [G,1,1,3,3]) -> channelAtt gate (sigmoid(gate_logits[b,g,y,x]) broadcast over the
 * disparities; NULL: no gate).  Bit-identical to ss_gwc_volume_fwd + ss_depthwise_patch_fwd.  Needs W % 4 == 0,
 * dmin % 4 == 0, ndisp % 8 == 0, C / groups in {4, 8}, 16-byte aligned pointers: SS_ERR_UNSUPPORTED otherwise (use the two calls). */
int ss_gwc_patch_gate_fwd(const float* ref, const float* tgt, const float* patch_w, const float* gate_logits, float* out,
                          int B, int C, int H, int W, int dmin, int ndisp, int groups, int normalize, ss_stream_t stream);
/* gradients of the UN-normalised volume w.r.t. ref and tgt (both fully written). */
int ss_gwc_volume_bwd(const float* grad_out, const float* ref, const float* tgt,
                      float* grad_ref, float* grad_tgt,
                      int B, int C, int H, int W, int dmin, int ndisp, int groups,
                      ss_stream_t stream);

/* build_concat_volume(ref, tgt, maxdisp)               models/submodule.py:173-187   (unsigned: models/submodule_.py:166-177)
 * out[b,0:C,p,y,x] = ref[b,:,y,x], out[b,C:2C,p,y,x] = tgt[b,:,y,x-(dmin+p)], 0 where the partner column leaves
 * the image -- in BOTH halves with mask_left != 0 (the signed form), in the right half only with mask_left == 0 (the
 * unsigned form copies the left image unmasked).  [B,C,H,W]^2 -> [B,2C,ndisp,H,W] */
int ss_concat_volume_fwd(const float* ref, const float* tgt, float* out,
                         int B, int C, int H, int W, int dmin, int ndisp, int mask_left, ss_stream_t stream);
int ss_concat_volume_bwd(const float* grad_out, float* grad_ref, float* grad_tgt,
                         int B, int C, int H, int W, int dmin, int ndisp, int mask_left, ss_stream_t stream);

/* SpatialTransformer_grid(x, y, disp_range_samples)    models/submodule.py:265-288
 * y_warped[b,c,j,h,w] = bilinear(y[b,c], row h, col w - disp[b,j,h,w]) with zeros padding and
 * align_corners=True, coordinates taken through the reference's normalise/unnormalise fp32
 * round trip; x_warped[b,c,j,h,w] = x[b,c,h,w].  x_warped may be NULL (not written).
 * x,y [B,C,H,W], disp [B,nd,H,W] -> [B,C,nd,H,W] each. */
int ss_warp_sampled_fwd(const float* x, const float* y, const float* disp,
                        float* y_warped, float* x_warped,
                        int B, int C, int H, int W, int nd, ss_stream_t stream);
/* its backward (autograd of the reference's meshgrid -> normalise -> F.grid_sample composition): grad_y_warped,
 * grad_x_warped [B,C,nd,H,W] (either may be NULL) -> grad_x = sum over the candidates of grad_x_warped, grad_y (scatter of
 * the bilinear weights; zeroed here, accumulated with fp32 atomics), grad_disp [B,nd,H,W] (the live use at
 * models/SemStereo.py:291, where the candidates derive from pred_att).  Outputs may be NULL when not needed. */
int ss_warp_sampled_bwd(const float* grad_y_warped, const float* grad_x_warped, const float* y, const float* disp,
                        float* grad_x, float* grad_y, float* grad_disp, int B, int C, int H, int W, int nd,
                        ss_stream_t stream);
/* Fused form of SemStereo.concat_volume_generator + `att_topk * volume`
 * (models/SemStereo.py:241-244, 318): out[b,0:C,j] = att[b,j] * left[b,:],
 * out[b,C:2C,j] = att[b,j] * warp(right)[b,:,j].  att [B,nd,H,W] may be NULL (no gating).
 * -> [B,2C,nd,H,W].  left == NULL: only the right half, -> [B,C,nd,H,W] (its left half then enters
 * concat_stem through ss_stem_left_fwd). */
int ss_concat_sampled_fwd(const float* left, const float* right, const float* disp, const float* att,
                          float* out, int B, int C, int H, int W, int nd, ss_stream_t stream);
/* (r06, training) Backward of ss_concat_sampled_fwd with both halves: grad_out [B,2C,nd,H,W] -> grad_left [B,C,H,W] (= sum_j att *
 * grad of the broadcast half), grad_right [B,C,H,W] (the warp's backward on att * grad of the warped half: bilinear taps of
 * F.grid_sample, zeros padding, align_corners=True as the forward) and grad_att [B,nd,H,W] (= sum_c grad . the ungated volume); any of
 * the three may be NULL; att may be NULL when grad_att is.  The candidates `disp` are constants (the indices of
 * models/SemStereo.py:299-305): no gradient.  `margin`: a bound on |disp| the caller expects (a performance hint: taps further away are
 * added one atomic at a time instead of through the LDS windows; any value gives the same result).  Any width: a
 * workgroup owns 64 columns of one row, the last block of a row may be partial (W % 64 == 0: whole blocks, the launch of the path's
 * own quarter-resolution widths).  SS_ERR_UNSUPPORTED beyond 2^31 - 1 such blocks (B * H * ceil(W / 64)). */
int ss_concat_sampled_bwd(const float* grad_out, const float* left, const float* right, const float* disp, const float* att,
                          float* grad_left, float* grad_right, float* grad_att, int B, int C, int H, int W, int nd, int margin,
                          ss_stream_t stream);
/* The right (warped) half of the same volume, att[b,j] * warp(right)[b,:,j] (models/SemStereo.py:241-244, 316-318), written
 * PRE-SPLIT for the matrix core: every value as the two fp16 terms of x * 2^(141 - e), 8 channels per 16-byte slot,
 *   xs [B][C/8][2 terms][nd][H][W][8] fp16 (C % 8 == 0, 4 bytes per value: the footprint of the fp32 volume),
 *   xexp int[3*B]: [0,B) the block exponent e of each batch element (from the bound max|right[b]| * max|att[b]|),
 *                  [B,3B) scratch for the two maxima.
 * Consumed by ss_conv3d_presplit_fwd, which stages it by LDS-DMA with no conversion.  att may be NULL. */
int ss_concat_sampled_presplit_fwd(const float* right, const float* disp, const float* att, void* xs, int* xexp,
                                   int B, int C, int H, int W, int nd, ss_stream_t stream);
/* The left (broadcast) half of concat_stem (models/SemStereo.py:319) by linearity:
 *   out[b,co,j,h,w] = sum_{kd,kh,kw} att[b, j+kd-1, h+kh-1, w+kw-1] * q[b, tap*Cout + co, h+kh-1, w+kw-1]
 * (zero outside), tap = kd*9+kh*3+kw, q [B,27*Cout,H,W] = the 1x1 convolution of the 2-D left concat
 * features with concat_stem's left-half weights (ss_conv3d_pointwise_bf16s_fwd), att [B,nd,H,W] the
 * top-k attention weights, out [B,Cout,nd,H,W]; nd in {6, 24, 32}, Cout % 4 == 0.  The result is the
 * `residual` operand of the right half's ss_conv3d[_bf16s]_fwd. */
int ss_stem_left_fwd(const float* q, const float* att, float* out, int B, int Cout, int nd, int H, int W,
                     ss_stream_t stream);
/* The same, with q computed on the fly on the matrix core and never written: left [B,C,H,W] (C = 32) is the
 * 2-D left concat feature map, wsplit = ss_pack_pointwise_weights_bf16s of the [Cout/2 * 64, C] matrix whose
 * row pair*64 + tap*2 + c is (scale *) W[2*pair + c, :C, tap] (rows 54-63 of every pair zero). */
int ss_stem_left_fused_fwd(const float* left, const void* wsplit, const float* att, float* out, int B, int C,
                           int Cout, int nd, int H, int W, int nterms, ss_stream_t stream);
/* The same on the two-term fp16 form (f16x3 engine), Q by shifts: per (kh, kw) the matrix product's B operand is the left
 * map's tile SHIFTED by that offset, so every lane receives the Q values of its own output and the 27 multiply-adds read
 * them from the accumulator registers (no Q tile in LDS).  C = Cout = 32, nd in {6, 24, 32}; anything else is
 * SS_ERR_UNSUPPORTED.  wsplit = ss_pack_stem_left_weights_f16s of the left-half weights w [Cout, C, 27] (tap = kd*9+kh*3+kw):
 * 73728 fp16 terms in fragment order (two terms of w / u, u a power of two per (tap, output channel)) followed by the 864
 * floats u; ss_pack_stem_left_weights_f16s_bytes, 16-byte aligned. */
int ss_stem_left_mfma_fwd(const float* left, const void* wsplit, const float* att, float* out, int B, int C,
                          int Cout, int nd, int H, int W, ss_stream_t stream);
int ss_pack_stem_left_weights_f16s(const float* w, void* wsplit, int Cout, int C, ss_stream_t stream);
/* Packed-weight sizes.  Every ss_pack_* entry point that fills a `void*` buffer of split fragments has a twin `<name>_bytes(<its
 * scalar arguments, same order>, long long* bytes)`: the bytes the pack writes and its consumer reads, from the one function in the
 * .hip file that owns the layout -- what a caller allocates.  No stream, no device.  A NULL `bytes` or a non-positive dimension:
 * SS_ERR_INVALID; arguments the pack refuses: the pack's own status; a refused call writes nothing. */
int ss_pack_stem_left_weights_f16s_bytes(int Cout, int C, long long* bytes);
/* Fused form of models/SemStereo.py:291-292: mean over channels of left * warp(right):
 * x,y [B,C,H,W], disp [B,nd,H,W] -> [B,nd,H,W] */
int ss_warp_correlation_fwd(const float* x, const float* y, const float* disp, float* out,
                            int B, int C, int H, int W, int nd, ss_stream_t stream);

/* disparity_regression(x, maxdisp)                     models/submodule.py:164-170   (unsigned: models/submodule_.py:159-163)
 * out[b,y,x] = sum_p prob[b,p,y,x] * (dmin + p), p in [0, ndisp).  [B,ndisp,H,W] -> [B,H,W] */
int ss_disparity_regression_fwd(const float* prob, float* out, int B, int dmin, int ndisp, int H, int W,
                                ss_stream_t stream);
int ss_disparity_regression_bwd(const float* grad_out, float* grad_prob, int B, int dmin, int ndisp, int H, int W,
                                ss_stream_t stream);
/* disparity_variance(x, maxdisp, disparity)            models/submodule.py:257-263   (unsigned: models/submodule_.py:239-245)
 * out[b,0,y,x] = sum_p prob[b,p,y,x] * ((dmin + p) - disparity[b,0,y,x])^2 */
int ss_disparity_variance_fwd(const float* prob, const float* disparity, float* out,
                              int B, int dmin, int ndisp, int H, int W, ss_stream_t stream);
/* Fused softmax over D + regression + variance of models/SemStereo.py:281-285:
 * logits [B,ndisp,H,W] -> prob (nullable) [B,ndisp,H,W], disp [B,H,W], var [B,1,H,W] */
int ss_softmax_regression_fwd(const float* logits, float* prob, float* disp, float* var,
                              int B, int dmin, int ndisp, int H, int W, ss_stream_t stream);
/* The same with the trilinear up-sampling in front of it fused in (models/SemStereo.py:279-285):
 * coarse [B,1,ndisp/2,H/2,W/2] = classif_att_'s output; up [B,ndisp,H,W] receives
 * F.interpolate(coarse, [ndisp,H,W], mode='trilinear') (align_corners=False, exact 2x in every dimension: H, W, ndisp
 * even), disp [B,H,W] and var [B,1,H,W] the soft-argmax and variance of softmax(up) over the disparity axis.  ndisp <= 128. */
int ss_upsample_softmax_regression_fwd(const float* coarse, float* up, float* disp, float* var,
                                       int B, int dmin, int ndisp, int H, int W, ss_stream_t stream);

/* Fused models/SemStereo.py:286-293 (variance gate, Propagation x2 [models/submodule.py:290-307],
 * 5-sample SpatialTransformer_grid, channel-mean correlation, softmax over the 5 samples):
 *   strength[b,t,y,x] = softmax_t( mean_c left[b,c,y,x] * warp(right, pred0[b,nb_t(y,x)])[c]
 *                                  * sigmoid(beta + gamma * var[b,0,nb_t(y,x)]) )
 * with nb_t the five replicate-padded diagonal neighbours.  left,right [B,C,H,W]; pred0 [B,H,W];
 * var [B,1,H,W]; gamma, beta: 1-element device arrays -> strength [B,5,H,W] */
int ss_sample_strength_fwd(const float* left, const float* right, const float* pred0, const float* var,
                           const float* gamma, const float* beta, float* strength,
                           int B, int C, int H, int W, ss_stream_t stream);
/* Fused models/SemStereo.py:295-310 (Propagation_prob [models/submodule.py:361-377] weighted by
 * strength, softmax over D, descending stable sort, top-k, ascending re-sort, gathers, softmax over
 * the k, expectation):  logits [B,1,ndisp,H,W], strength [B,5,H,W] ->
 *   samples [B,k,H,W] (candidate disparities dmin + index, ascending, as floats), att_topk [B,1,k,H,W] (their
 *   probabilities), pred_att [B,H,W].  ndisp <= 128. */
int ss_topk_candidates_fwd(const float* logits, const float* strength, float* samples, float* att_topk,
                           float* pred_att, int B, int dmin, int ndisp, int H, int W, int k, ss_stream_t stream);

/* regression_topk(cost, disparity_samples, k)         models/submodule.py:434-442
 * per pixel: the k largest costs (ties: lower index first), softmax over them, expectation of
 * the matching candidates.  cost, samples [B,nd,H,W] -> [B,1,H,W].  1 <= k <= min(nd, 32). */
int ss_regression_topk_fwd(const float* cost, const float* samples, float* out,
                           int B, int nd, int H, int W, int k, ss_stream_t stream);
/* its backward: grad_out [B,1,H,W] -> grad_cost, grad_samples [B,nd,H,W] (fully written; zero outside the k selected
 * candidates; no gradient through the selection itself, as autograd of the reference's sort/gather composition gives). */
int ss_regression_topk_bwd(const float* grad_out, const float* cost, const float* samples, float* grad_cost,
                           float* grad_samples, int B, int nd, int H, int W, int k, ss_stream_t stream);

/* SSR_upsample.forward(depth_low, weights, pred_label)   models/submodule.py:412-431 (calls: SemStereo.py:311, 324)
 * 4x bilinear up-sampling of the 1/4-scale disparity + class-probability-gated residual, one kernel.
 *   depth_low [B,1,h,w]; weights (spx_pred), pred_label [B,n,4h,4w]; out [B,4h,4w]; n = 6.
 *   params: ss_ssr_param_count() floats (153 since ABI 12) = the module's parameters with every eval-mode BatchNorm2d
 *   FOLDED into the convolution before it and the two gate stages pre-multiplied by -log2(e), packed as laid out at the top of
 *   csrc/ssr_upsample.hip (semstereo_amd/modules.py: SSR_upsample._params packs it, in float64). */
int ss_ssr_upsample_fwd(const float* depth_low, const float* weights, const float* pred_label,
                        const float* params, float* out, int B, int h, int w, int num_classes,
                        ss_stream_t stream);
int ss_ssr_param_count(void);
/* (ABI 20) Its training form, forward and backward on the HIP kernels (csrc/ssr_upsample_train.hip): BatchNorm on batch statistics
 * (batch_stats = 1: nn.Module.train(), models/submodule.py:412-431 as main_us3d.py:198-206 trains it) or on the running statistics
 * (batch_stats = 0: eval() under autograd).  n = num_classes = 6 only (SS_ERR_UNSUPPORTED otherwise).
 *   params: the head's 16 parameter tensors flattened in nn.Module.parameters() order (189 floats: conv.0.weight/bias,
 *     conv.1.weight/bias, conv.2.weight/bias, conv1.0.weight/bias, conv1.1.weight/bias, conv2.0.weight/bias, conv2.1.weight/bias,
 *     conv3.weight/bias); grad_params has the same layout and is fully written by the backward.
 *   saved: 256 floats, 8-byte aligned, written by the forward (float64 mean / invstd of BN0 = conv.0, BNa = conv.2, BN1 = conv1.1,
 *     BN2 = conv2.1 and the statistics folded into the convolutions) and read by the backward of the same call.
 *   running statistics (rm*, rv*, nbt*: conv.0, conv.2, conv1.1, conv2.1): with batch_stats = 1 moved inside the kernels as
 *     F.batch_norm moves them (momentum per layer, variance unbiased, num_batches_tracked += 1; a NULL pointer is left alone);
 *     with batch_stats = 0 rm* / rv* are the statistics used (required) and nothing is written.
 *   workspace: float64-aligned scratch of at least 8 * 128 * G bytes (forward) or 8 * 128 * G + 256 + (grad_depth_low ? 28 * N : 0)
 *     bytes (backward), N = B * 16 * h * w, G = min(ceil(N / 256), 1024).
 *   grad_depth_low [B,1,h,w], grad_weights / grad_pred_label [B,n,4h,4w]: each NULL = not wanted (not computed / written).
 * Sums are per-workgroup float64 partials summed in a fixed order: results are bitwise reproducible run to run. */
int ss_ssr_upsample_train_fwd(const float* depth_low, const float* weights, const float* pred_label, const float* params,
                              float* out, float* saved, float* rm0, float* rv0, long long* nbt0, float* rma, float* rva,
                              long long* nbta, float* rm1, float* rv1, long long* nbt1, float* rm2, float* rv2, long long* nbt2,
                              float eps0, float epsa, float eps1, float eps2, double mom0, double moma, double mom1, double mom2,
                              int batch_stats, int B, int h, int w, int num_classes, double* workspace, long long workspace_bytes,
                              ss_stream_t stream);
int ss_ssr_upsample_train_bwd(const float* depth_low, const float* weights, const float* pred_label, const float* params,
                              const float* saved, const float* grad_out, float* grad_depth_low, float* grad_weights,
                              float* grad_pred_label, float* grad_params, int batch_stats, int B, int h, int w, int num_classes,
                              double* workspace, long long workspace_bytes, ss_stream_t stream);

/* channelAtt gating (models/SemStereo.py:101-102): out[b,c,d,y,x] = sigmoid(att[b,c,y,x]) * cv[b,c,d,y,x] */
int ss_channel_gate_fwd(const float* att_logits, const float* cv, float* out,
                        int B, int C, int D, int H, int W, ss_stream_t stream);

/* channelAtt.im_att (models/SemStereo.py:89-100; BasicConv, models/submodule.py:89-116) in one launch:
 *   out[b,cv,y,x] = W2[cv,:] . relu(scale1 * (W1 . im[b,:,y,x]) + shift1) + bias2[cv]     (sigmoid of it when `sigmoid`)
 * im [B,Cin,H,W]; w1_split / w2_split: W1 [Cmid,Cin], W2 [Cout,Cmid] packed by ss_pack_pointwise_weights_bf16s;
 * scale1 / shift1: the eval-mode BatchNorm2d folded to an affine (NULL: identity); bias2 may be NULL.
 * Built for the reference's two gates: (Cin, Cmid, Cout) = (256, 128, 32) and (128, 64, 32). */
int ss_channel_att_logits_fwd(const float* im, const void* w1_split, const float* scale1, const float* shift1,
                              const void* w2_split, const float* bias2, float* out,
                              int B, int Cin, int Cmid, int Cout, int H, int W, int sigmoid, ss_stream_t stream);

/* ---- 3-D aggregation stack -------------------------------------------------------------
 * Conv3d(bias=False) [+ BatchNorm3d in eval] [+ residual] [+ ReLU]: convbn_3d
 * (models/submodule_other.py:845-848), BasicConv(is_3d) (models/submodule.py:89-116), the
 * classifier heads (models/SemStereo.py:228-234).
 *   in      [B,Cin,D,H,W]
 *   wpack   weights re-laid out as [Cin][kd*kh*kw][Cout] (see ss_pack_conv3d_weights)
 *   scale, shift   per-Cout affine applied to the accumulator (folded BN; NULL = 1 / 0)
 *   residual       [B,Cout,Do,Ho,Wo] added after the affine (NULL = none)
 *   relu           != 0 -> max(.,0)
 *   gate           [B,Cout,Ho,Wo] channelAtt gate, already sigmoid-activated (models/SemStereo.py:101-102):
 *                  the result is multiplied by it, broadcast over D, last (NULL = none)
 *   kernel k in {1,3} (cubic), stride in {1,2}, pad = k/2.  out [B,Cout,Do,Ho,Wo],
 *   Do = (D + 2*pad - k)/stride + 1 ... */
int ss_conv3d_fwd(const float* in, const float* wpack, const float* scale, const float* shift,
                  const float* residual, const float* gate, float* out,
                  int B, int Cin, int D, int H, int W, int Cout, int k, int stride, int relu,
                  ss_stream_t stream);
/* Same contract as ss_conv3d_fwd for k = 3, stride 1, computed on the bf16 matrix core with every fp32
 * operand split exactly into three bf16 terms ("split-bf16"): nterms = 6 keeps all cross terms down to
 * 2^-24 (measured error below the exact-fp32 MFMA's, tools/exp_split_bf16.hip), nterms = 3 keeps
 * hi*hi + hi*mid + mid*hi.  wsplit comes from ss_pack_conv3d_weights_bf16s (16-byte aligned).
 * stride in {1, 2}. */
int ss_conv3d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                        const float* residual, const float* gate, float* out,
                        int B, int Cin, int D, int H, int W, int Cout, int stride, int relu, int nterms,
                        ss_stream_t stream);
/* The same convolution continuing a PARTIAL SUM: out = gate * relu?(scale * (partial + conv(in)) + shift), partial
 * [B,Cout,D,H,W] = the contribution of input channels that are not in `in` (ss_stem_left_fused_fwd: the broadcast
 * half of concat_stem's input).  It initialises the accumulators, read under the first chunk's staging. */
int ss_conv3d_bf16s_partial_fwd(const float* in, const void* wsplit, const float* partial, const float* scale,
                                const float* shift, const float* gate, float* out,
                                int B, int Cin, int D, int H, int W, int Cout, int relu, int nterms,
                                ss_stream_t stream);
/* concat_stem with the warped half of the sparse concat volume formed INSIDE the convolution's staging (round 5; SURVEY.md
 * section 8 f1, second half).  Replaces, in one launch and without a [B,Cin,nd,H,W] volume,
 *   models/SemStereo.py:241-244 (concat_volume_generator: SpatialTransformer_grid, models/submodule.py:265-288),
 *   :318 (att_topk * volume) on the warped half, :319 (concat_stem: Conv3d k3 s1 p1 + BatchNorm + ReLU over THESE Cin channels,
 *   continuing `partial`) and :320 (the channelAtt gate):
 *   out[b,co,j,h,w] = gate[b,co,h,w] * relu?(scale[co] * (partial[b,co,j,h,w] + sum_{ci,taps} w * x[b,ci,j',h',w']) + shift[co]),
 *   x[b,ci,j,h,w] = att[b,j,h,w] * right[b,ci,h,w - cand[b,j,h,w]]  (0 where that column lies outside [0,W)).
 * right [B,Cin,H,W]; cand, att [B,nd,H,W]; partial [B,Cout,nd,H,W] / scale / shift [Cout] / gate [B,Cout,H,W] may be NULL.
 * CONTRACT: the candidates are INTEGER-valued floats -- what models/SemStereo.py:299-305 produces (indices - maxdisp/4) --
 * for which the reference's bilinear F.grid_sample is a gather up to its own coordinate rounding (<= 1e-5 relative on the
 * columns / rows whose normalise -> unnormalise round trip is inexact; the gather is the float64-exact value).  Fractional
 * candidates are truncated toward zero: use ss_concat_sampled_fwd + ss_conv3d_bf16s_partial_fwd for those.
 * Cin % 8 == 0, Cin >= 16; nterms = 19 only (wsplit from ss_pack_conv3d_weights_f16s); SS_ERR_UNSUPPORTED otherwise. */
int ss_conv3d_gather_fwd(const float* right, const float* cand, const float* att, const void* wsplit, const float* partial,
                         const float* scale, const float* shift, const float* gate, float* out,
                         int B, int Cin, int nd, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream);
/* concat_stem on the pre-split warped half (models/SemStereo.py:319-320): Conv3d(k3, s1, p1, bias=False) over
 * xs / xexp of ss_concat_sampled_presplit_fwd (Cin % 8 == 0), out = gate * relu?(scale * (partial + conv) + shift);
 * wsplit from ss_pack_conv3d_weights_f16s; partial [B,Cout,D,H,W], scale / shift [Cout], gate [B,Cout,H,W] may be NULL.
 * Same results contract as ss_conv3d_bf16s_partial_fwd with nterms = 19 (the block exponent is per batch element
 * instead of per staged tile). */
int ss_conv3d_presplit_fwd(const void* xs, const int* xexp, const void* wsplit, const float* partial, const float* scale,
                           const float* shift, const float* gate, float* out, int B, int Cin, int D, int H, int W,
                           int Cout, int relu, ss_stream_t stream);
/* Conv3d weight [Cout,Cin,3,3,3] fp32 -> split/packed bf16 fragments
 * [ceil(Cin/8)][14 tap pairs][3 terms][2 halves][Cout][8] (ss_pack_conv3d_weights_bf16s_bytes). */
int ss_pack_conv3d_weights_bf16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv3d_weights_bf16s_bytes(int Cout, int Cin, long long* bytes);
/* The two-term fp16 form of the same layers (same reference lines): ss_conv3d_bf16s_fwd / _partial_fwd with
 * nterms = 19 ("f16x3": hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, half the matrix-core time of nterms = 6).
 * fp16 has 5 exponent bits, so the operands are block floating point: this packer scales each output channel's weights
 * by a power of two (stored behind the terms and undone in the epilogue), the kernel scales every staged 8-channel chunk
 * of its halo tile by a power of two taken from the tile's running |max| and rescales its fp32 accumulators when it
 * changes.  Error vs exact: representation <= 2^-23 per operand + the dropped lo*lo <= 2^-22 per product, i.e. below
 * the fp32 accumulation error of any K >= 64 (measured in DESIGN.md section 4).  wsplit:
 * [ceil(Cin/8)][14][2 terms][2 halves][Cout][8] fp16 + float[Cout]  (ss_pack_conv3d_weights_f16s_bytes). */
int ss_pack_conv3d_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv3d_weights_f16s_bytes(int Cout, int Cin, long long* bytes);
/* The 2-D form of the split-bf16 conv: Conv2d(k3, s1, p1, bias=False) + affine (+residual) + ReLU on [B,Cin,H,W] maps
 * (concat_feature, models/SemStereo.py:222-226): out [B,Cout,H,W]; w [Cout,Cin,3,3] -> wsplit
 * [ceil(Cin/8)][5 tap pairs][3 terms][2 halves][Cout][8] (ss_pack_conv2d_weights_bf16s_bytes). */
int ss_conv2d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                        const float* residual, float* out, int B, int Cin, int H, int W, int Cout, int relu,
                        int nterms, ss_stream_t stream);
/* The same layer on TWO input tensors in one launch: out [2B,Cout,H,W], elements 0..B-1 from in_a, B..2B-1 from in_b (both
 * [B,Cin,H,W]) -- `concat_feature` applied to the left and to the right view (models/SemStereo.py:314-315) without a torch.cat
 * in front and with twice the workgroups per launch (round 5).  No residual operand. */
int ss_conv2d_bf16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale, const float* shift,
                             float* out, int B, int Cin, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream);
int ss_pack_conv2d_weights_bf16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv2d_weights_bf16s_bytes(int Cout, int Cin, long long* bytes);
/* The same layer with its input given as TWO channel ranges: channels [0, Csplit) from x_a [B,Csplit,H,W], [Csplit, Cin) from
 * rem_a [B,Cin-Csplit,H,W] -- Conv2x's `torch.cat((x, rem), 1)` + conv2 (models/submodule.py:156-160) without the concatenated
 * tensor.  x_b / rem_b (both or neither): a second view in the same launch (FeatUp applies each Conv2x to the left view, then to the
 * right one, models/SemStereo.py:74-84): out [2B,Cout,H,W], elements 0..B-1 from the _a pair, B..2B-1 from the _b pair; NULL:
 * out [B,Cout,H,W].  wsplit is the plain form's (ss_pack_conv2d_weights_f16s / _bf16s of the [Cout,Cin,3,3] weight), and the result
 * is bit-identical to ss_conv2d_bf16s_fwd on the materialised concatenation at the same launch batch (2B with two views).  As in that
 * entry point the tile depends on the launch's batch, so two views in one launch may differ from two single launches in the last bits.
 * Csplit % 8 == 0, else SS_ERR_UNSUPPORTED. */
int ss_conv2d_bf16s_cat_fwd(const float* x_a, const float* rem_a, const float* x_b, const float* rem_b, const void* wsplit,
                            const float* scale, const float* shift, float* out, int B, int Csplit, int Cin, int H, int W, int Cout,
                            int relu, int nterms, ss_stream_t stream);
/* ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) + per-channel affine + optional ReLU on [B,Cin,H,W] maps -> out [B,Cout,2H,2W]:
 * conv1 of every 2-D Conv2x (BasicConv(deconv=True): ConvTranspose2d(bias=False) + BatchNorm2d + ReLU, models/submodule.py:89-116,
 * 136-138, 150 -- FeatUp's deconv32_16 .. deconv4_2, models/SemStereo.py:63-66, and spx32_16 .. spx4_2, :208-211) with the eval
 * BatchNorm folded into (scale, shift), and `spx2` (nn.ConvTranspose2d(128, 6, 4, 2, 1) with a bias, models/SemStereo.py:207, 271:
 * scale NULL, shift = the bias, relu 0).  Four output-parity classes, each a 2x2 convolution (K = 4 Cin) on the two-term fp16
 * form of the matrix-core engine: nterms must be 19 (anything else: SS_ERR_UNSUPPORTED).  scale / shift may be NULL (1 / 0).
 * wsplit from ss_pack_deconv2d_weights_f16s.  out must be 8-byte aligned. */
int ss_deconv2d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out, int B, int Cin,
                          int H, int W, int Cout, int relu, int nterms, ss_stream_t stream);
/* The same layer on TWO input tensors in one launch (the two views of FeatUp.forward, models/SemStereo.py:74-84): out
 * [2B,Cout,2H,2W], elements 0..B-1 from in_a, B..2B-1 from in_b (both [B,Cin,H,W]); every element gets the bits a single launch
 * gives it. */
int ss_deconv2d_bf16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale, const float* shift,
                               float* out, int B, int Cin, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream);
/* nn.ConvTranspose2d weight [Cin,Cout,4,4] fp32 (models/submodule.py:104) -> the fragments of ss_deconv2d_bf16s_fwd:
 * [ceil(Cin/8)][ceil(Cout/32)][4 parity classes][2 tap rows][2 terms][2 tap columns][32 channels][8] fp16 of w scaled per output
 * channel by a power of two, + float[32 ceil(Cout/32)] of the inverse scales (ss_pack_deconv2d_weights_f16s_bytes), 16-byte aligned. */
int ss_pack_deconv2d_weights_f16s(const float* w, void* wsplit, int Cin, int Cout, ss_stream_t stream);
int ss_pack_deconv2d_weights_f16s_bytes(int Cin, int Cout, long long* bytes);
/* (training) The data gradient of ConvTranspose2d(k = 4, s = 2, p = 1) -- conv1 of every 2-D Conv2x (models/submodule.py:104,
 * 136-138, 150) and `spx2` (models/SemStereo.py:207) -- as what it is: Conv2d(Cin, Cout, 4, stride=2, padding=1, bias=False) on
 * in [B,Cin,H,W] (the gradient of the transposed conv's output; H and W even, else SS_ERR_UNSUPPORTED) -> out [B,Cout,H/2,W/2], the
 * transposed conv's own weight tensor read as [Cout,Cin,4,4] (no flip).  Two-term fp16 form of the matrix-core engine
 * (csrc/deconv2d_train.hip); no affine, no ReLU.  The tile is chosen per layer: an element has the same bits alone and in a batch.
 * An infinity in `in` reaches its own receptive field only.  wsplit from ss_pack_conv2d_k4s2_weights_f16s.  One element's input or
 * output of 2 GiB or more: SS_ERR_UNSUPPORTED. */
int ss_conv2d_k4s2_f16s_fwd(const float* in, const void* wsplit, float* out, int B, int Cin, int H, int W, int Cout, ss_stream_t stream);
/* Conv2d weight [Cout,Cin,4,4] fp32 (= nn.ConvTranspose2d's [its Cin, its Cout, 4, 4], models/submodule.py:104) -> the fragments of
 * ss_conv2d_k4s2_f16s_fwd: [ceil(Cin/8)][ceil(Cout/32)][8 K-steps][2 terms][2 lane halves][32 channels][8] fp16 of w scaled per output
 * channel by a power of two, + float[32 ceil(Cout/32)] of the inverse scales (ss_pack_conv2d_k4s2_weights_f16s_bytes), 16-byte aligned. */
int ss_pack_conv2d_k4s2_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv2d_k4s2_weights_f16s_bytes(int Cout, int Cin, long long* bytes);
/* (training) The weight gradient of the same layer (models/submodule.py:104, 136-138, 150; models/SemStereo.py:207):
 * grad_w[ci,co,kh,kw] = sum_{b,y,x} in[b,ci,y,x] * grad_out[b,co,2y-1+kh,2x-1+kw], in [B,Cin,H,W], grad_out [B,Cout,2H,2W], grad_w
 * [Cin,Cout,4,4].  Three-term bf16 form, six products, fp32 accumulation; one partial [16][32][32] block per workgroup in `workspace`
 * (ss_deconv2d_k4s2_wgrad_workspace_bytes) and a fixed-order final sum in double: no floating-point atomics, the same inputs give
 * the same bits.  One element's tensors of 2 GiB or more: SS_ERR_UNSUPPORTED. */
int ss_deconv2d_k4s2_wgrad_fwd(const float* in, const float* grad_out, float* grad_w, float* workspace, int B, int Cin, int H, int W,
                               int Cout, ss_stream_t stream);
/* Its workspace: nparts * ceil(Cin/32) * ceil(Cout/32) * 65536 bytes, where with rows = B * H and tiles = ceil(Cin/32) * ceil(Cout/32)
 * a partial covers rpp = min(rows, max(ceil(rows / clamp(1024 / tiles, 1, 256)), ceil(2048 / W))) rows and nparts = ceil(rows / rpp):
 * at most max(64 MiB, tiles * 64 KiB) -- 64 MiB up to 1024 weight tiles, one partial per tile beyond.  A refused call writes nothing. */
int ss_deconv2d_k4s2_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, long long* bytes);
/* (training) The weight gradient of Conv2d(C0 + C1, Cout, 3, stride 1, padding 1, bias=False) applied to cat((in0, in1), 1), the
 * concatenation never formed -- conv2 of every 2-D Conv2x (models/submodule.py:142, 157-160), `concat_feature`
 * (models/SemStereo.py:221-223) and the 3x3 conv1 of `segmenthead` (the class whose forward is models/submodule.py:40-52):
 * grad_w[co,ci,kh,kw] = sum_{b,y,x} grad_out[b,co,y,x] * in[b,ci,y+kh-1,x+kw-1] with zero padding; grad_out [B,Cout,H,W], in0
 * [B,C0,H,W], in1 [B,C1,H,W]; channels ci < C0 are read from in0, the rest from in1; grad_w [Cout,C0+C1,3,3] is written whole, never
 * accumulated into.  C1 == 0 with in1 == NULL is the single-source form (C1 > 0 with in1 == NULL, C1 < 0: SS_ERR_INVALID).  Three-term
 * bf16 form, six products, fp32 accumulation (the arithmetic and order of ss_deconv2d_k4s2_wgrad_fwd); operands staged through LDS
 * and split once, the grad_out row shared by the three kh waves, each input row staged once per workgroup; one partial [9][32][32]
 * block per workgroup in `workspace` (ss_conv2d_k3_wgrad_workspace_bytes) and a fixed-order final sum in double: no floating-point
 * atomics, the same inputs give the same bits.  One element's grad_out, in0 or in1 of 2 GiB or more, B * H beyond an int, more than
 * 65535 weight tiles: SS_ERR_UNSUPPORTED. */
int ss_conv2d_k3_wgrad_fwd(const float* grad_out, const float* in0, const float* in1, float* grad_w, float* workspace, int B, int C0,
                           int C1, int H, int W, int Cout, ss_stream_t stream);
/* Its workspace: nparts * tiles * 36864 bytes, where with rows = B * H and tiles = (ceil(C0/32) + ceil(C1/32)) * ceil(Cout/32) a
 * partial covers rpp = min(rows, max(ceil(rows / clamp(1024 / tiles, 1, 256)), ceil(2048 / W))) rows and nparts = ceil(rows / rpp):
 * at most max(36 MiB, tiles * 36 KiB).  A refused call writes nothing. */
int ss_conv2d_k3_wgrad_workspace_bytes(int B, int C0, int C1, int H, int W, int Cout, long long* bytes);
/* Conv2d(Cin, Cout, 1) + per-channel affine + optional ReLU on [B,Cin,npos] maps (npos = H*W) -> out [B,Cout,npos]: the projections
 * `chal_0 .. chal_4` = nn.Sequential(nn.Conv2d(1x1, bias), nn.BatchNorm2d) (models/SemStereo.py:213-217, called at :258-262), with
 * the bias and the eval BatchNorm folded into (scale, shift), on the two-term fp16 form of the matrix-core engine with a loop over
 * Cin: any Cin % 8 == 0 (else SS_ERR_UNSUPPORTED), any Cout >= 1.  A workgroup owns 64 consecutive positions of one element
 * whatever the batch: an element has the same bits alone, in a batch and in the pair form.  scale / shift may be NULL (1 / 0).
 * wsplit from ss_pack_conv2d_k1_weights_f16s.  One element's input and output must stay below 2 GiB (SS_ERR_UNSUPPORTED). */
int ss_conv2d_k1_f16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out, int B, int Cin,
                          long long npos, int Cout, int relu, ss_stream_t stream);
/* The same layer on TWO input tensors in one launch (chal_1 / chal_2 on the left and on the right view, models/SemStereo.py:259-260,
 * 264-265): out [2B,Cout,npos], elements 0..B-1 from in_a, B..2B-1 from in_b (both [B,Cin,npos]). */
int ss_conv2d_k1_f16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale, const float* shift,
                               float* out, int B, int Cin, long long npos, int Cout, int relu, ss_stream_t stream);
/* nn.Conv2d weight [Cout,Cin,1,1] fp32 (models/SemStereo.py:213-217) -> the fragments of ss_conv2d_k1_f16s_fwd:
 * [ceil(Cin/32)][ceil(Cout/32)][2 K-steps][2 terms][2 channel octets][32 output channels][8] fp16 of w scaled per output channel by
 * a power of two, + float[32 ceil(Cout/32)] of the inverse scales (ss_pack_conv2d_k1_weights_f16s_bytes), 16-byte aligned. */
int ss_pack_conv2d_k1_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv2d_k1_weights_f16s_bytes(int Cout, int Cin, long long* bytes);
/* The segmentation head up to its logits (segmenthead.forward, models/submodule.py:42-44: conv1 = BasicConv(Cin, 32, 3x3, padding 1)
 * = Conv2d(bias=False) + BatchNorm2d + ReLU, :89-116, then conv2 = nn.Conv2d(32, K, 1, bias=True); `head_l` / `head_r`,
 * models/SemStereo.py:200-201, 254-255) in one pass: the 32-channel map stays in the accumulators.  in [B,Cin,H,W], Cin % 8 == 0;
 * (scale, shift) the folded eval BatchNorm of conv1 (NULL: 1 / 0); w2 [K,32], bias [K], K <= 8; out [B,K,H,W].  wsplit from
 * ss_pack_seghead_weights_f16s.  The tile is 8 x 32 positions of one element whatever the batch. */
int ss_seghead_logits_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, const float* w2,
                          const float* bias, float* out, int B, int Cin, int H, int W, int K, ss_stream_t stream);
/* conv1.conv.weight [32,Cin,3,3] fp32 -> the fragments of ss_seghead_logits_fwd: [Cin/8][5 K-steps][2 terms][2 taps][32 channels][8]
 * fp16 + float[32] inverse scales (ss_pack_seghead_weights_f16s_bytes), 16-byte aligned.  Cin % 8 == 0. */
int ss_pack_seghead_weights_f16s(const float* w, void* wsplit, int Cin, ss_stream_t stream);
int ss_pack_seghead_weights_f16s_bytes(int Cin, long long* bytes);
/* F.interpolate(in, size=(2H, 2W), mode="bilinear", align_corners=False) of [B,C,H,W] -> [B,C,2H,2W] (segmenthead.forward with
 * scale_factor 2, models/submodule.py:46-51): weights 0.25 / 0.75, source index clamped at the borders, horizontal pair first. */
int ss_bilinear_up2_fwd(const float* in, float* out, int B, int C, int H, int W, ss_stream_t stream);
/* (training) The head's tail under autograd (csrc/seghead_train.hip): out = up2(w2 . a + bias) in one pass, the low-resolution logits
 * never written.  a [B,K,H,W]: the head's 32-channel map after BatchNorm + ReLU; w2 [C,K], bias [C]: conv2's parameters; out
 * [B,C,sH,sW], s = 1 + up2; up2 = 1: F.interpolate(size=(2H, 2W), mode="bilinear", align_corners=False) with the arithmetic of
 * ss_bilinear_up2_fwd, up2 = 0 (scale_factor None): the 1x1 + bias alone.  K = 32 and C <= 8 (SS_ERR_UNSUPPORTED otherwise, and for
 * one element's `a` or `out` of 2 GiB or more).  The tile is 8 x 32 positions of one element whatever the batch. */
int ss_seghead_tail_fwd(const float* a, const float* w2, const float* bias, float* out, int B, int K, int C, int H, int W, int up2,
                        ss_stream_t stream);
/* Its backward in one pass over grad_out [B,C,sH,sW]: g = the adjoint of the up-sampling (G read at the clamped index), then
 * grad_a [B,K,H,W] = w2^T g, grad_w2 [C,K] = sum g a, grad_bias [C] = sum g.  Any of the three may be NULL (not computed), not all.
 * The two sums go through one partial per workgroup in `workspace` (ss_seghead_tail_workspace_bytes; may be NULL when both are) and a
 * fixed-order final sum in double: no floating-point atomics, the same inputs give the same bits. */
int ss_seghead_tail_bwd(const float* grad_out, const float* a, const float* w2, float* grad_a, float* grad_w2, float* grad_bias,
                        float* workspace, int B, int K, int C, int H, int W, int up2, ss_stream_t stream);
int ss_seghead_tail_workspace_bytes(int B, int K, int C, int H, int W, long long* bytes);
/* two-term fp16 form of the 2-D weights (nterms = 19 of ss_conv2d_bf16s_fwd; see ss_pack_conv3d_weights_f16s):
 * [ceil(Cin/8)][5][2 terms][2 halves][Cout][8] fp16 + float[Cout] (ss_pack_conv2d_weights_f16s_bytes). */
int ss_pack_conv2d_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_conv2d_weights_f16s_bytes(int Cout, int Cin, long long* bytes);
/* The single-output-channel classifier heads, nn.Conv3d(C, 1, 3, padding=1, bias=False)
 * (models/SemStereo.py:228-234, classif.2 / classif_att_.2), on the split-bf16 engine with the 27 taps as
 * the matrix rows:  out [B,1,D,H,W] = relu?(scale[0] * conv(in [B,Cin,D,H,W]) + shift[0]);
 * Cin in {16, 32, 64}; nterms 6 / 3: wsplit from ss_pack_conv3d_head_weights_bf16s ([Cin/16][3 terms][2 k-halves][32 rows][8] bf16:
 * ss_pack_conv3d_head_weights_bf16s_bytes); nterms 19: from ss_pack_conv3d_head_weights_f16s. */
int ss_conv3d_head_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                             float* out, int B, int Cin, int D, int H, int W, int relu, int nterms,
                             ss_stream_t stream);
int ss_pack_conv3d_head_weights_bf16s(const float* w, void* wsplit, int Cin, ss_stream_t stream);
int ss_pack_conv3d_head_weights_bf16s_bytes(int Cin, long long* bytes);
/* nterms = 19 of the two head entry points: two fp16 terms, three products, block floating point (one power-of-two scale
 * for the weights, one per input row from a wave-wide maximum) -- half the matrix work of nterms = 6 at the same accuracy
 * class.  wsplit: [Cin/16][2 terms][2 k-halves][32 rows][8] fp16 + one float (2^-scale) in a 16-byte tail
 * (ss_pack_conv3d_head_weights_f16s_bytes). */
int ss_pack_conv3d_head_weights_f16s(const float* w, void* wsplit, int Cin, ss_stream_t stream);
int ss_pack_conv3d_head_weights_f16s_bytes(int Cin, long long* bytes);
/* The two layers of a classifier (nn.Sequential(convbn_3d(32,32,3,1,1), ReLU, Conv3d(32,1,3,p1)), models/SemStereo.py:228-234)
 * hand their intermediate over CHANNELS-LAST, [B][D][H][W][C]: it is private to the Sequential, and with a position's
 * channels contiguous the first layer stores 16 bytes per lane and instruction and the head loads 16 (the head spends half
 * of its time issuing 4-byte loads otherwise).  ss_conv3d_bf16s_cl_fwd = ss_conv3d_bf16s_fwd (stride 1, no residual, no
 * gate, Cout % 8 == 0) with that output layout; ss_conv3d_head_bf16s_cl_fwd = ss_conv3d_head_bf16s_fwd reading it
 * (Cin = 32, `in` 16-byte aligned).  Same arithmetic, same results as the plain-layout pair. */
int ss_conv3d_bf16s_cl_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out,
                           int B, int Cin, int D, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream);
int ss_conv3d_head_bf16s_cl_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                                float* out, int B, int Cin, int D, int H, int W, int relu, int nterms,
                                ss_stream_t stream);
/* The same classifier in ONE pass over the volume (r05): the 32-channel intermediate never leaves the CU.  The first layer's
 * tile (4 planes x 4 rows x 32 columns x 32 channels) contracts its ReLU(BN(conv)) with the head's 27 x 32 weights on the matrix
 * core as soon as its K loop ends, sums the 27 shifted tap images over the tile in a fixed order and writes the tile's
 * contribution to the 6 x 6 x 34 output positions it touches -- a PATCH -- into `patches`
 * ([B][ceil(W/32) * ceil(H/4) * D/4][6*6*34] floats, caller-allocated scratch); a second small launch adds the <= 8 patches that
 * hold an output position, again in a fixed order: deterministic, and a pair gets the same bits at every batch size.
 *   head_w: ss_pack_classifier_head_weights(w2 [1,32,3,3,3]) -> [3 bf16 terms][2 K-steps][64 lanes][8]
 *   (ss_pack_classifier_head_weights_bytes), 16-byte aligned.
 * Cin % 8 == 0, 32 intermediate channels, nterms = 19, D % 4 == 0 and a layer of at least 512 (2 x 8 x 32) tiles per pair;
 * anything else returns SS_ERR_UNSUPPORTED (the caller keeps the two-launch form above).  y is the two-launch form's y bit for
 * bit; the head's 864 products per output are summed in another order (within fp32 rounding of it). */
int ss_pack_classifier_head_weights(const float* w2, void* out, ss_stream_t stream);
int ss_pack_classifier_head_weights_bytes(long long* bytes);
int ss_conv3d_classifier_fused_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                                   const void* head_w, float* patches, float* out, int B, int Cin, int D, int H, int W,
                                   int nterms, ss_stream_t stream);
/* regression_topk(cost.squeeze(1), samples, 2) (models/SemStereo.py:322-323, models/submodule.py:434-442) reading the patches of
 * ss_conv3d_classifier_fused_fwd directly (call that with out = NULL: no patch-sum launch, no [B,1,nd,H,W] cost tensor): patches
 * [B][tiles][1224], samples [B,nd,H,W] -> out [B,1,H,W], bit-identical to the two-launch form.  nd = 24 and k = 2 (the model's);
 * anything else returns SS_ERR_UNSUPPORTED. */
int ss_regression_topk_patched_fwd(const float* patches, const float* samples, float* out, int B, int nd, int H, int W, int k,
                                   ss_stream_t stream);
/* 1x1x1 Conv3d / per-position Linear (+ per-channel affine: bias; ReLU) on the split-bf16 engine:
 * qkv_3d and final1x1 of attention_block (models/submodule_other.py:804, 835).
 *   out [B,Cout,npos] = relu?(scale * (W in) + shift), in [B,Cin,npos], npos = D*H*W, W [Cout,Cin];
 * Cin in {32, 64, 128}; wsplit from ss_pack_pointwise_weights_bf16s
 * ([ceil(Cout/32)][Cin/16][3 terms][2 k-halves][32 rows][8] bf16: ss_pack_pointwise_weights_bf16s_bytes). */
int ss_conv3d_pointwise_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                                  float* out, int B, int Cin, int Cout, long long npos, int relu, int nterms,
                                  ss_stream_t stream);
int ss_pack_pointwise_weights_bf16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream);
int ss_pack_pointwise_weights_bf16s_bytes(int Cout, int Cin, long long* bytes);

/* ConvTranspose3d(k3, s2, p1, output_padding 1, bias=False) [+BN] fused with the 1x1x1 skip
 * projection of hourglass.forward (models/SemStereo.py:141-142):
 *   out = relu?( scale*deconv(in) + shift + skip_scale*conv1x1(skip) + skip_shift )
 *   in [B,Cin,D,H,W] -> out [B,Cout,2D,2H,2W]; wpack [Cin][27][Cout] (tap = kd*9+kh*3+kw of
 *   the ConvTranspose3d weight [Cin,Cout,3,3,3]); skip [B,Cs,2D,2H,2W] with skip_wpack
 *   [Cs][Cout] (NULL skip = plain deconv+affine). */
int ss_deconv3d_fwd(const float* in, const float* wpack, const float* scale, const float* shift,
                    const float* skip, const float* skip_wpack, const float* skip_scale, const float* skip_shift,
                    float* out, int B, int Cin, int D, int H, int W, int Cout, int Cs, int relu,
                    ss_stream_t stream);
/* The same layer on the split-bf16 engine (deconv3d_bf16s.hip): wsplit / skip_wsplit come from
 * ss_pack_deconv3d_weights_bf16s applied to the fp32 packs of ss_deconv3d_fwd (wpack [Cin][27][Cout] with the
 * BatchNorm scale folded, ntaps = 27; skip_wpack [Cs][Cout], ntaps = 1); only a common shift is applied.
 * wsplit: [ceil(Cin/16)][ntaps][3 terms][2 channel halves][Cout][8] bf16 (ss_pack_deconv3d_weights_bf16s_bytes). */
int ss_deconv3d_bf16s_fwd(const float* in, const void* wsplit, const float* shift, const float* skip,
                          const void* skip_wsplit, float* out, int B, int Cin, int D, int H, int W, int Cout,
                          int Cs, int relu, int nterms, ss_stream_t stream);
/* ... preceded by a 1x1x1 conv WITH BIAS that has been folded into it (hourglass.forward: attention_block.final1x1 into
 * conv5): wsplit packs the composed weights W'[ci][tap][co] = sum_m Wo[m][ci] W5[m][tap][co] (BN scale folded), and the bias,
 * carried through the transposed conv, is a constant per output channel AND border case of the output position --
 * shift27 [27][Cout], row (cd * 3 + ch) * 3 + cw with per axis 0 = even output index, 1 = odd interior, 2 = the last odd
 * index 2N - 1 -- with the layer's own common shift already added.  The skip projection is required. */
int ss_deconv3d_bf16s_shift27_fwd(const float* in, const void* wsplit, const float* shift27, const float* skip,
                                  const void* skip_wsplit, float* out, int B, int Cin, int D, int H, int W, int Cout,
                                  int Cs, int relu, int nterms, ss_stream_t stream);
int ss_pack_deconv3d_weights_bf16s(const float* wpack, void* wsplit, int Cin, int Cout, int ntaps, ss_stream_t stream);
int ss_pack_deconv3d_weights_bf16s_bytes(int Cin, int Cout, int ntaps, long long* bytes);
/* Two-term fp16 form of the MAIN weights (ntaps = 27) for nterms = 19 of ss_deconv3d_bf16s_fwd -- the block-floating
 * scheme described at ss_pack_conv3d_weights_f16s; the skip projection keeps its bf16 pack.
 * wsplit: [ceil(Cin/16)][27][2 terms][2 channel halves][Cout][8] fp16 + float[Cout] (ss_pack_deconv3d_weights_f16s_bytes). */
int ss_pack_deconv3d_weights_f16s(const float* wpack, void* wsplit, int Cin, int Cout, ss_stream_t stream);
int ss_pack_deconv3d_weights_f16s_bytes(int Cin, int Cout, long long* bytes);
/* Weight re-layout helpers (device to device): Conv3d weight [Cout,Cin,k,k,k] or
 * ConvTranspose3d weight [Cin,Cout,k,k,k] (transposed != 0) -> [Cin][k^3][Cout]. */
int ss_pack_conv3d_weights(const float* w, float* wpack, int Cout, int Cin, int k, int transposed,
                           ss_stream_t stream);
/* Weight gradient of Conv3d(k3, padding 1, stride 1 | 2, bias=False) -- the training path, main_us3d.py:186-222:
 *   grad_w[co,ci,kd,kh,kw] = sum_{b,od,oh,ow} grad_out[b,co,od,oh,ow] * in[b,ci,od*s+kd-1,oh*s+kh-1,ow*s+kw-1]
 * grad_out [B,Cout,Do,Ho,Wo], in [B,Cin,D,H,W] -> grad_w [Cout,Cin,3,3,3] (zeroed here, accumulated with fp32 atomics).
 * Also the weight gradient of ConvTranspose3d(k3,s2,p1,op1): call it with grad_out := the layer's input, in := the
 * gradient of its output, stride 2; the result is in that weight's [Cin,Cout,3,3,3] layout.  (The data gradients are the
 * forward entry points: ss_conv3d_bf16s_fwd on flipped weights / ss_deconv3d_fwd / the stride-2 convolution.) */
int ss_conv3d_wgrad_fwd(const float* grad_out, const float* in, float* grad_w, int B, int Cin, int D, int H, int W,
                        int Cout, int stride, ss_stream_t stream);
/* The same weight gradient on the bf16 matrix core (r06; conv3d_wgrad_bf16s.hip): both operands split exactly into three bf16
 * terms, six cross products on v_mfma_f32_32x32x16_bf16, fp32 accumulation (error below the exact-fp32 MFMA's, any magnitude
 * of gradient: bf16 has fp32's exponent range).  `workspace`: ceil(Cout/32) * ceil(Cin/32) * 27 * 1024 floats of scratch
 * (zeroed here; the waves' accumulator tiles are summed into it with coalesced fp32 atomics and re-ordered into grad_w, which is
 * written, not accumulated).  Same arguments and the same ConvTranspose3d convention as ss_conv3d_wgrad_fwd. */
int ss_conv3d_wgrad_bf16s_fwd(const float* grad_out, const float* in, float* grad_w, float* workspace, int B, int Cin, int D, int H,
                              int W, int Cout, int stride, ss_stream_t stream);

/* `patch` (models/SemStereo.py:219, 274): depthwise Conv3d kernel (1,3,3), pad (0,1,1), no bias,
 * optionally fused with the channelAtt gate that follows it (:276):
 *   out[b,c,d] = sigmoid?(gate[b,c]) * conv2d_3x3(in[b,c,d], w[c])       w [C,1,1,3,3], gate [B,C,H,W] or NULL */
int ss_depthwise_patch_fwd(const float* in, const float* w, const float* gate, float* out,
                           int B, int C, int D, int H, int W, ss_stream_t stream);
/* attention_block.forward (models/submodule_other.py:790-837): windowed multi-head
 * self-attention over (bd,bh,bw) windows + 1x1x1 conv with bias.
 *   x [B,C,D,H,W] (C = heads * 8), wqkv_t [C][3C] (= qkv_3d.weight transposed), bqkv [3C],
 *   wout_t [C][C] (= final1x1.weight[:, :, 0,0,0] transposed), bout [C] -> out [B,C,D,H,W].
 *   D % bd == 0; H, W are padded virtually to window multiples with the reference's masking. */
int ss_window_attention_fwd(const float* x, const float* wqkv_t, const float* bqkv,
                            const float* wout_t, const float* bout, float* out,
                            int B, int C, int D, int H, int W, int heads, int bd, int bh, int bw,
                            ss_stream_t stream);
/* The attention core alone, for the three-launch form of the same block: qkv [B,3C,D,H,W] is the
 * qkv_3d projection (+bias) of the UNPADDED volume (a 1x1x1 ss_conv3d_fwd), bqkv [3C] the value a
 * zero-padded token projects to; y [B,C,D,H,W] = softmax(q k^T / sqrt(hd) [+ pad mask]) v per window and
 * head, un-partitioned and cropped (models/submodule_other.py:805-834); final1x1 is another
 * ss_conv3d_fwd.  One workgroup per (window, 4 heads). */
int ss_window_attention_core_fwd(const float* qkv, const float* bqkv, float* y, int B, int C, int D, int H,
                                 int W, int heads, int bd, int bh, int bw, ss_stream_t stream);
/* The core with the qkv_3d projection inside: x [B,C,D,H,W] is the block's input, wqkv_split the [3C,C] weight packed by
 * ss_pack_pointwise_weights_bf16s, nterms 6 or 3 as for ss_conv3d_pointwise_bf16s_fwd.  Each (window, 4 heads) workgroup
 * projects its own q/k/v slab with that launch's arithmetic (same fragments, K-steps and product order), so y holds the
 * bits of ss_conv3d_pointwise_bf16s_fwd + ss_window_attention_core_fwd without the [B,3C,D,H,W] tensor between them. */
int ss_window_attention_proj_fwd(const float* x, const void* wqkv_split, const float* bqkv, float* y, int B, int C,
                                 int D, int H, int W, int heads, int bd, int bh, int bw, int nterms,
                                 ss_stream_t stream);

/* ---- training side of the 3-D stack (main_us3d.py:186-222): what the matrix-core forward / dgrad / wgrad kernels leave over ---- */
/* BatchNorm with BATCH statistics + optional ReLU (convbn_3d, models/submodule_other.py:845-848; BasicConv,
 * models/submodule.py:89-116, in train()): x [B,C,N] (N = D*H*W or H*W), weight / bias [C] or NULL -> y, and mean / invstd /
 * var_unbiased [C] (for the backward and the running statistics).  work: 2*C doubles of scratch. */
int ss_batchnorm_train_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean, float* invstd,
                           float* var_unbiased, double* work, int B, int C, long long N, float eps, int relu,
                           ss_stream_t stream);
/* ... backward: grad_x [B,C,N]; grad_bias[c] = work[2c], grad_weight[c] = work[2c+1] (doubles).  y is read only when relu. */
int ss_batchnorm_train_bwd(const float* grad_y, const float* x, const float* y, const float* mean, const float* invstd,
                           const float* weight, float* grad_x, double* work, int B, int C, long long N, int relu,
                           ss_stream_t stream);
/* The same pair with a residual joining behind the normalisation and before the ReLU: y = relu(bn(x) + residual) -- the
 * `F.relu(self.conv5(conv4) + self.redir2(conv2))` of hourglass.forward in train() (models/SemStereo.py:141-142) in one pass;
 * backward: also grad_residual [B,C,N] = grad_y behind the ReLU mask. */
int ss_batchnorm_train_res_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* y, float* mean,
                               float* invstd, float* var_unbiased, double* work, int B, int C, long long N, float eps, int relu,
                               ss_stream_t stream);
int ss_batchnorm_train_res_bwd(const float* grad_y, const float* x, const float* y, const float* mean, const float* invstd,
                               const float* weight, float* grad_x, float* grad_residual, double* work, int B, int C, long long N,
                               int relu, ss_stream_t stream);
/* BatchNorm on its RUNNING statistics under autograd (a module in eval() whose inputs / parameters require gradients; the reference's
 * training loop never freezes BatchNorm, main_us3d.py:186-222, PyTorch allows it): forward with the caller's per-channel mean and
 * invstd = 1 / sqrt(running_var + eps), optional residual (joins before the ReLU) and ReLU; backward: grad_x = w * invstd * g'
 * (g' = grad_y behind the ReLU mask), grad_residual = g' when not NULL, grad_bias[c] = work[2c], grad_weight[c] = work[2c + 1]. */
int ss_batchnorm_eval_fwd(const float* x, const float* residual, const float* mean, const float* invstd, const float* weight,
                          const float* bias, float* y, int B, int C, long long N, int relu, ss_stream_t stream);
int ss_batchnorm_eval_bwd(const float* grad_y, const float* x, const float* y, const float* mean, const float* invstd,
                          const float* weight, float* grad_x, float* grad_residual, double* work, int B, int C, long long N,
                          int relu, ss_stream_t stream);
/* (r06) The batch-statistics forward, either form (residual may be NULL), that also does nn.BatchNorm's bookkeeping in its statistics
 * kernel: running_mean / running_var [C] (NULL = leave alone) become running * (1 - momentum) + momentum * batch value (the variance
 * unbiased) as F.batch_norm moves them (torch/nn/modules/batchnorm.py: the reference's layers keep the default momentum 0.1), and
 * num_batches_tracked (int64[1] or NULL) counts the batch.  0 <= momentum <= 1; a module with momentum=None (cumulative average) is not
 * this entry's case. */
int ss_batchnorm_train_fwd_rs(const float* x, const float* residual, const float* weight, const float* bias, float* y, float* mean,
                              float* invstd, float* var_unbiased, double* work, float* running_mean, float* running_var,
                              long long* num_batches_tracked, double momentum, int B, int C, long long N, float eps, int relu,
                              ss_stream_t stream);
/* (r06) Both backward forms with the parameter gradients also as floats, grad_weight / grad_bias [C] (either may be NULL; the doubles
 * stay in `work`); grad_residual may be NULL; batch_statistics = 1: the backward of ss_batchnorm_train_fwd / _res_fwd / _fwd_rs,
 * 0: of ss_batchnorm_eval_fwd.  `bias`: the forward's (NULL = none).  y may be NULL where the forward had a ReLU and no residual: the
 * mask is recomputed from x with the forward's own expression, and y is not read (two of the backward's seven tensor passes). */
int ss_batchnorm_bwd_pg(const float* grad_y, const float* x, const float* y, const float* mean, const float* invstd,
                        const float* weight, const float* bias, float* grad_x, float* grad_residual, double* work, float* grad_weight,
                        float* grad_bias, int batch_statistics, int B, int C, long long N, int relu, ss_stream_t stream);
/* (r06, training) The normalisation of groupwise_correlation_norm (models/submodule.py:213-222), once per feature map:
 * y = x / (||x||_2 over each group's C / groups channels + eps), x [B,C,H,W]; and its backward (grad_x from grad_y and x).  The
 * volume is then built from the normalised maps by ss_gwc_volume_fwd / _bwd. */
int ss_group_normalise_fwd(const float* x, float* y, int B, int C, int H, int W, int groups, float eps, ss_stream_t stream);
int ss_group_normalise_bwd(const float* grad_y, const float* x, float* grad_x, int B, int C, int H, int W, int groups, float eps,
                           ss_stream_t stream);
/* Weight gradient of the 1x1(x1) convolutions (redir1 / redir2 `models/SemStereo.py:131-132`, attention_block.qkv_3d /
 * final1x1 `models/submodule_other.py:799-800`, channelAtt.im_att `models/SemStereo.py:92-95`):
 * grad_out [B,Cout,npos], in [B,Cin,npos] -> grad_w [Cout,Cin]. */
int ss_conv_k1_wgrad_fwd(const float* grad_out, const float* in, float* grad_w, int B, int Cin, int Cout, long long npos,
                         ss_stream_t stream);
/* sums[c] (double) = sum over batch and positions of a[b,c,:]: bias gradients of the 1x1x1 projections of attention_block
 * (models/submodule_other.py:799-800). */
int ss_channel_sum_fwd(const float* a, double* sums, int B, int C, long long N, ss_stream_t stream);
/* Weight gradient of `patch` (depthwise Conv3d (1,3,3), models/SemStereo.py:219): grad_w [C,1,1,3,3]. */
int ss_depthwise_patch_wgrad_fwd(const float* grad_out, const float* in, float* grad_w, int B, int C, int D, int H, int W,
                                 ss_stream_t stream);
/* channelAtt's gate (models/SemStereo.py:101-102), gradient of the logits:
 * grad_att [B,C,H,W] = s (1 - s) * sum_d grad_out[b,c,d] * cv[b,c,d], s = sigmoid(att_logits).  (The gradient of cv is
 * ss_channel_gate_fwd applied to grad_out.) */
int ss_channel_gate_bwd_logits(const float* grad_out, const float* cv, const float* att_logits, float* grad_att, int B, int C,
                               int D, int H, int W, ss_stream_t stream);
/* Backward of ss_window_attention_core_fwd (models/submodule_other.py:805-834) for volumes whose H, W are multiples of
 * the window (no pad tokens): qkv [B,3C,D,H,W], grad_y [B,C,D,H,W] -> grad_qkv [B,3C,D,H,W]. */
int ss_window_attention_core_bwd(const float* qkv, const float* grad_y, float* grad_qkv, int B, int C, int D, int H, int W,
                                 int heads, int bd, int bh, int bw, ss_stream_t stream);
/* ... for any H, W (r04): the reference zero-pads the volume BEFORE the qkv Linear (models/submodule_other.py:808-813), so a pad
 * token's q / k / v are that Linear's bias `bqkv` [3C] (the qkv tensor holds real positions only), its output is cropped, and a logit
 * between a pad and a real token carries -1000 when BOTH H and W were padded (:822-829).  grad_bias [3C] (zeroed by the call) receives
 * what reaches the pad tokens' q / k / v: the extra term of the Linear's bias gradient. */
int ss_window_attention_core_pad_bwd(const float* qkv, const float* bqkv, const float* grad_y, float* grad_qkv, float* grad_bias, int B,
                                     int C, int D, int H, int W, int heads, int bd, int bh, int bw, ss_stream_t stream);
/* Backward of the three fused attention-tail launches (training; models/SemStereo.py:279-310 under autograd; r04).  Each recomputes
 * its forward quantities from the saved inputs.  Gradient outputs that are scattered into neighbouring pixels (fp32 atomics) are
 * zeroed by the call; any gradient input / output pointer may be NULL unless said otherwise.
 *   ss_upsample_softmax_regression_bwd  :279-285  up [B,1,D,H,W] (the forward's output), grad_up / grad_disp [B,H,W] / grad_var [B,1,H,W]
 *                                                 -> grad_coarse [B,1,D/2,H/2,W/2] (required); work: B*D*H*W floats of scratch
 *   ss_sample_strength_bwd              :286-293  grad_strength [B,5,H,W] (required) -> grad_left / grad_right [B,C,H,W], grad_pred0 [B,H,W],
 *                                                 grad_var [B,1,H,W], grad_gamma_beta [2]
 *   ss_topk_candidates_bwd              :295-310  samples [B,K,H,W] = the forward's selection; grad_att_topk [B,1,K,H,W], grad_pred_att [B,H,W]
 *                                                 -> grad_logits [B,1,D,H,W], grad_strength [B,5,H,W] */
int ss_upsample_softmax_regression_bwd(const float* up, const float* grad_up, const float* grad_disp, const float* grad_var,
                                       float* grad_coarse, float* work, int B, int dmin, int ndisp, int H, int W, ss_stream_t stream);
int ss_sample_strength_bwd(const float* left, const float* right, const float* pred0, const float* var, const float* gamma,
                           const float* beta, const float* grad_strength, float* grad_left, float* grad_right, float* grad_pred0,
                           float* grad_var, float* grad_gamma_beta, int B, int C, int H, int W, ss_stream_t stream);
/* ... through a scratch `work` of B * 5 * H * W floats: two launches, the channels on the second one's grid (r06: 3x faster at 128 channels) */
int ss_sample_strength_bwd_ws(const float* left, const float* right, const float* pred0, const float* var, const float* gamma,
                              const float* beta, const float* grad_strength, float* grad_left, float* grad_right, float* grad_pred0,
                              float* grad_var, float* grad_gamma_beta, float* work, int B, int C, int H, int W, ss_stream_t stream);
int ss_topk_candidates_bwd(const float* logits, const float* strength, const float* samples, const float* grad_att_topk,
                           const float* grad_pred_att, float* grad_logits, float* grad_strength, int B, int dmin, int ndisp, int H, int W,
                           int k, ss_stream_t stream);
/* ---- the training objective (main_us3d.py:199-208; models/loss.py), csrc/loss.hip ----
 * Streaming reductions without floating-point atomics: the same inputs give the same bits.  Every result stays on the device: `loss` is
 * one float, `record` the sums the backward reads (doubles).  `workspace`: ss_loss_workspace_bytes(kind) bytes of scratch, kind 0 = the
 * disparity loss, 1 = the label / LRSC loss.  Nothing is allocated, copied or synchronised inside. */
int ss_loss_workspace_bytes(int kind, long long* bytes);
/* model_loss_train / model_loss_test (models/loss.py:19-31): loss = sum_i w_i * mean over the kept pixels of smooth-L1 (beta 1; l1 = 1:
 * |.|) of est_i - gt_i, nterms <= 4 terms of n_i elements in one launch.  A pixel is kept where mask_i (a bool tensor) is set or, with
 * mask_i NULL, where lo <= gt_i < hi (how main_us3d.py:199-200 forms its masks).  record [8]: per term the kept sum and the kept count.
 * An empty selection gives 0 / 0 = NaN, as PyTorch's mean does. */
int ss_disparity_loss_fwd(const float* est0, const float* gt0, const unsigned char* mask0, long long n0, const float* est1,
                          const float* gt1, const unsigned char* mask1, long long n1, const float* est2, const float* gt2,
                          const unsigned char* mask2, long long n2, const float* est3, const float* gt3, const unsigned char* mask3,
                          long long n3, float w0, float w1, float w2, float w3, float lo, float hi, int nterms, int l1, double* record,
                          float* loss, double* workspace, long long workspace_bytes, ss_stream_t stream);
/* ... backward: grad_i = grad_loss * w_i * clamp(est_i - gt_i, -1, 1) / count_i on kept pixels (sign for l1), 0 elsewhere; grad_i NULL:
 * that estimate asks for none.  grad_loss: one float on the device. */
int ss_disparity_loss_bwd(const float* est0, const float* gt0, const unsigned char* mask0, float* grad0, long long n0, const float* est1,
                          const float* gt1, const unsigned char* mask1, float* grad1, long long n1, const float* est2, const float* gt2,
                          const unsigned char* mask2, float* grad2, long long n2, const float* est3, const float* gt3,
                          const unsigned char* mask3, float* grad3, long long n3, float w0, float w1, float w2, float w3, float lo,
                          float hi, int nterms, int l1, const double* record, const float* grad_loss, ss_stream_t stream);
/* model_label_loss (models/loss.py:106-119 with dice_loss :33-63): scale * (cross-entropy ignoring class `ignore` + 1 - Dice over batch,
 * classes 0..C-2 and pixels), logits [B,C,H,W] with C = 6, labels [B,H,W] of label_dtype 0 = int64, 1 = uint8, 2 = float32 (integer
 * values).  A label outside [0, C) counts as ignored.  record [5]: sum (lse - z_y) over counted pixels, their count, sum p_y over
 * y < C-1, sum (1 - p_{C-1}), count of y < C-1. */
int ss_label_loss_fwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W, int ignore, float scale,
                      double* record, float* loss, double* workspace, long long workspace_bytes, ss_stream_t stream);
/* ... backward: recomputes the softmax, reads the record; grad_logits [B,C,H,W]. */
int ss_label_loss_bwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W, int ignore, float scale,
                      const double* record, const float* grad_loss, float* grad_logits, ss_stream_t stream);
/* LRSC_loss (models/loss.py:121-135): plain cross-entropy of the right view's logits against the left labels gathered at column
 * (long) clamp((float) x - disp[b,h,x], 0, W - 1) of the same row, evaluated in fp32 as the reference's tensor expression is.  The same
 * kernels in their gather mode.  warped (optional, int64 [B,H,W]): the gathered label map.  The disparity gets no gradient. */
int ss_lrsc_loss_fwd(const float* logits_right, const float* disp, const void* labels, int label_dtype, int B, int num_classes, int H, int W,
                     double* record, float* loss, long long* warped, double* workspace, long long workspace_bytes, ss_stream_t stream);
int ss_lrsc_loss_bwd(const float* logits_right, const float* disp, const void* labels, int label_dtype, int B, int num_classes, int H, int W,
                     const double* record, const float* grad_loss, float* grad_logits, ss_stream_t stream);
/* ---- the evaluation step's metrics (main_us3d.py:225-263; utils/metrics.py), csrc/metrics.hip ----
 * Streaming reductions like the objective's: integer counts, the error sum in double from the wave on, one partial per workgroup, a
 * second small launch that adds them in a fixed order.  No floating-point atomics, nothing comes back to the host.  `workspace`:
 * ss_metrics_workspace_bytes(kind) bytes of scratch, kind 0 = the disparity metrics, 1 = the confusion matrix. */
int ss_metrics_workspace_bytes(int kind, long long* bytes);
/* EPE_metric / D1_metric / Thres_metric with their per-image wrapper (utils/metrics.py:16-59) and the *_mask variants (:63-89), for
 * n_est <= 4 estimates [B, pixels_per_image] that share one ground truth, in one pass.  mask (bool) or, with mask NULL, lo <= gt < hi
 * (main_us3d.py:235) decides which images are skipped (n_mask / n_pos < 0.1, n_pos = #(gt > 0)); the selected pixels are those of
 * mask_img (bool) or, with mask_img NULL, of the mask.  E = |gt - est| in fp32.
 *   out    [n_est][2 + n_thr] floats: mean over the kept images of  mean E,  mean (E > 3 & E / |gt| > 0.05),  mean (E > t_k), k < n_thr <= 4;
 *          0 where no image is kept, NaN where a kept image has an empty selection
 *   counts [n_est][B][8] int64: n_sel, n_mask, n_pos, n_d1, n_thr[4];   sums [n_est][B] doubles: sum of E over the selection */
int ss_disparity_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, const float* gt,
                             const unsigned char* mask, const unsigned char* mask_img, int n_est, int B, long long pixels_per_image,
                             float lo, float hi, float t0, float t1, float t2, float t3, int n_thr, float* out, long long* counts,
                             double* sums, void* workspace, long long workspace_bytes, ss_stream_t stream);
/* SegmentationMetric.get_confusion_matrix (utils/metrics.py:143-168) without its host copy: the joint histogram joint[g][p], int64
 * [7][6], of the label class g (6 = outside [0, 6)) and p = the first maximum over the 6 channels of logits [B,6,H,W] (a NaN counts as
 * the maximum, as in np.argmax).  labels: label_dtype 0 = int64, 1 = uint8, 2 = float32 (truncated toward zero), pixel (b, h, x) at
 * b * label_image_stride + h * label_row_stride + x elements, so a label tensor larger than the logits is cropped without a copy.
 * accumulate != 0: the counts are added to `joint` (addBatch over an epoch); else `joint` is written.  Other class counts: -2. */
int ss_seg_confusion_fwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W,
                         long long label_row_stride, long long label_image_stride, long long* joint, int accumulate, void* workspace,
                         long long workspace_bytes, ss_stream_t stream);
/* ---- the joint stereo-semantic record (disparity error per semantic class, mIoU-3), csrc/joint_metrics.hip ----
 * One more streaming reduction of the same kind, over the tensors the two calls above read, once: n_est <= 4 estimates [B,H,W] against
 * gt; the mask (bool) or, with mask NULL, lo <= gt < hi; labels decoded exactly as in ss_seg_confusion_fwd (dtype codes, strides, class
 * g in [0, 6) or 6 = outside); logits [B,6,H,W] with p = their first maximum, or NULL: the three joint tables are not produced and
 * may be NULL.  E = |gt - est| in fp32; d1 = E > 3 & E / |gt| > 0.05; thr_k = E > t_k, k < n_thr <= 4; good = in the mask & E < tau
 * (E == tau and a NaN E are not good).  All outputs are PER IMAGE, so the caller applies the skip rule and accumulates on the device:
 *   image      [B][2] int64             n_mask, n_pos (= #(gt > 0))
 *   cls_sel    [B][7] int64             pixels in the mask, per class
 *   cls_counts [n_est][B][7][5] int64   n_d1, n_thr[4] of the pixels in the mask, per class
 *   cls_sums   [n_est][B][7] doubles    sum of E over them (fp32 values added in double from the thread on)
 *   joint_all, joint_out [B][7][6] int64   every pixel / the pixels outside the mask, by (g, p)
 *   joint_good [n_est][B][7][6] int64   the good pixels (bad = all - out - good)
 * Integer counts are exact; one partial per workgroup, a second launch adds them in a fixed order; no floating-point atomics.
 * workspace: ss_joint_metrics_scratch(n_est, B) bytes.  num_classes != 6, more than 1024 images, H W >= 2^31 - 1: -2. */
int ss_joint_metrics_scratch(int n_est, int B, long long* bytes);
int ss_joint_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, const float* gt,
                         const unsigned char* mask, const float* logits, const void* labels, int label_dtype, long long label_row_stride,
                         long long label_image_stride, int n_est, int B, int num_classes, int H, int W, float lo, float hi, float t0,
                         float t1, float t2, float t3, int n_thr, float tau, long long* image, long long* cls_sel, long long* cls_counts,
                         double* cls_sums, long long* joint_all, long long* joint_out, long long* joint_good, void* workspace,
                         long long workspace_bytes, ss_stream_t stream);
/* ---- the evaluation step's image outputs (main_us3d.py:252, :265-268; main_whu.py:242, :250-251), csrc/vis.hip ----
 * Streaming passes without atomics: a lane takes 4 consecutive pixels of a row (16-byte accesses where the address allows), results are
 * planar [B,3,H,W], element offsets are 64-bit, every division is the IEEE one.  Nothing comes back to the host.  A map of 2^31 or more
 * 4-pixel groups: -2.  ss_vis_workspace_bytes(kind) bytes of scratch, kind 0 = ss_image_minmax_fwd (the other calls need none). */
int ss_vis_workspace_bytes(int kind, long long* bytes);
/* disp_error_image_func.forward (utils/visualization.py:30-55) without its host copies and its twenty boolean-mask passes: est, gt
 * [B,H,W] fp32 -> out [B,3,H,W] fp32.  e = min(|gt - est| / abs_thres, (|gt - est| / gt) / rel_thres) in fp32 (a NaN in either term
 * gives NaN, as np.minimum); the pixel takes colour i of `table` where table[i][0] <= e < table[i][1], and black where gt is not valid
 * or no row matches (NaN, +inf).  table: HOST memory, 10 rows of {lo, hi, r, g, b} floats -- gen_error_colormap() (:11-24) cast to
 * float32 -- read during the call and passed to the kernel by value.  legend != 0: rows < 10, columns 20 i .. 20 i + 19 take colour i
 * (:51-53), clipped to H and W, also where gt is not valid.  Valid: gt > 0 (:36); with is_signed != 0: lo <= gt < hi and gt != 0, the
 * relative term over |gt| -- the signed disparities of US3D, where the reference's rule paints every negative ground truth black. */
int ss_disp_error_image_fwd(const float* est, const float* gt, const float* table, int B, int H, int W, float abs_thres, float rel_thres,
                            int legend, int is_signed, float lo, float hi, float* out, ss_stream_t stream);
/* feature_vis (utils/mask_vis.py:5-31) without its host copy, and the same picture straight from a label map, for which the scripts
 * build F.one_hot(label, 6).permute().float() only to take its argmax (main_us3d.py:266).  src_dtype -1: src = logits [B,C,H,W] fp32,
 * C = num_classes <= 6 (more: -2); the class is the first maximum over the channels, a NaN counting as the maximum (np.argmax, as in
 * ss_seg_confusion_fwd).  src_dtype 0 = int64, 1 = uint8, 2 = float32 (truncated toward zero): src = labels, pixel (b, h, x) at
 * b * label_image_stride + h * label_row_stride + x elements (the strides are ignored for logits).  out [B,3,H,W], out_dtype 0 = float32,
 * 1 = uint8, holds the palette of :10-15 with the values 0 and 255; a label outside [0, 6) gives black (the reference raises). */
int ss_class_color_fwd(const void* src, int src_dtype, int B, int num_classes, int H, int W, long long label_row_stride,
                       long long label_image_stride, void* out, int out_dtype, ss_stream_t stream);
/* The per-image range that save_images (utils/experiment.py:84-99) asks of make_grid(normalize=True, scale_each=True):
 * minmax[b] = {min, max} over the elements_per_image floats of image b.  Wave, LDS, one partial per workgroup in `workspace`, then a
 * second small launch that reads the partials in a fixed order: the same bits on every call.  More than 1024 images: -2. */
int ss_image_minmax_fwd(const float* x, int B, long long elements_per_image, float* minmax, void* workspace, long long workspace_bytes,
                        ss_stream_t stream);
/* ... and the normalisation itself: out = (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5f) in fp32 with {lo, hi} = minmax[b], x [B,C,P]
 * with P = pixels_per_channel.  out is [B,C,P], or [B,3,P] with three equal channels for C = 1 (make_grid's single-channel rule).
 * More than 65535 images: -2. */
int ss_image_normalize_fwd(const float* x, const float* minmax, float* out, int B, int C, long long pixels_per_channel, ss_stream_t stream);
/* ---- sample preparation (datasets/us3d_.py:70-215, datasets/whu_dataset.py:42-92, datasets/data_io.py:6-13), csrc/sample_prep.hip ----
 * What the reference's __getitem__ computes on the host for every item, from the raw arrays on the device.  Streaming passes: a lane
 * takes 4 consecutive pixels of a row, wide accesses where the address allows.  No atomics.  Nothing comes back to the host.  A tensor
 * of 2^31 or more elements: -2.
 * ss_prep_workspace_bytes: scratch of the luma / gradient pair for a [B,H,W] batch -- integer partial sums, then the uint8 luma plane. */
int ss_prep_workspace_bytes(int B, int H, int W, long long* bytes);
/* ToTensor + Normalize of both views: left, right uint8 [B,H,W,3] -> out_left, out_right float32 [B,3,H,W], out[b][c][y][x] =
 * table[c][u].  table: DEVICE memory, float [3][256], (u / 255 - mean[c]) / std[c] built by the caller in fp32 with the constants of
 * data_io.py:7-8 -- no division runs here.  right and out_right may both be NULL (one view). */
int ss_prep_views_fwd(const unsigned char* left, const unsigned char* right, const float* table, int B, int H, int W, float* out_left,
                      float* out_right, ss_stream_t stream);
/* cv2.resize(a, (w // k, h // k), INTER_NEAREST) for every requested level in one launch, H and W divisible by 16 (other sizes: -2): the
 * source pixel of (y, x) is (y k, x k).  disparity [B,H,W] contiguous, disp_dtype 0 = float32, 1 = int32; every disparity output is
 * float(v) * disp_scale in fp32 (WHU: 1 / 256, exact).  label: label_dtype 0 = int64, 1 = uint8, 2 = float32, pixel (b, h, x) at
 * b * label_image_stride + h * label_row_stride + x elements; every label output is the value widened to float32.  Outputs:
 * disparity_out, label_out [B,H,W]; disparity_k, label_k [B,H/k,W/k].  A NULL output is skipped; a source is read only where sampled
 * and may be NULL if none of its outputs is asked for. */
int ss_prep_pyramid_fwd(const void* disparity, int disp_dtype, float disp_scale, const void* label, int label_dtype,
                        long long label_row_stride, long long label_image_stride, int B, int H, int W, float* disparity_out,
                        float* disparity_4, float* disparity_8, float* disparity_16, float* label_out, float* label_2, float* label_4,
                        ss_stream_t stream);
/* PIL's convert("L") of left uint8 [B,H,W,3], L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, written as a uint8 plane into
 * `workspace` together with the parts of S1 = sum L and S2 = sum L^2 per image as 64-bit integers (wave, LDS, one partial pair per
 * workgroup; the gradient pass adds them: integer sums, exact in any order, so two calls give the same bits).  H W > 2^23 (where
 * N S2 - S1^2 leaves 64 bits) or more than 65535 images: -2. */
int ss_prep_luma_stats_fwd(const unsigned char* left, int B, int H, int W, void* workspace, long long workspace_bytes, ss_stream_t stream);
/* gx, gy float32 [B,1,H,W] of the dataset (us3d_.py:98-109) from the workspace that ss_prep_luma_stats_fwd filled on the same stream:
 * mean = S1 / N, std = sqrt(N S2 - S1^2) / N, z[L] = (L - mean) / std in double (a 256-entry table per image in LDS),
 * gx = float(z(y, x-1) - z(y, x+1)), gy = float(z(y-1, x) - z(y+1, x)), zero outside the image (convolve2d flips the kernel).  The
 * centre tap 0 * z(y, x) is kept: a constant image (std = 0) is NaN on every pixel, as in the reference. */
int ss_prep_gradients_fwd(const void* workspace, long long workspace_bytes, int B, int H, int W, float* gx, float* gy, ss_stream_t stream);
/* ---- right-view ground truth and the left-right consistency check, csrc/right_view.hip ----
 * The forward warp the reference left as a commented-out per-pixel loop (datasets/us3d_.py:115-133, "label_r" at :193) and that
 * LRSC_loss (models/loss.py:121-135) stands in for.  Row-wise, per image and row; d = disparity [B,H,W] float32 of the LEFT view, a left
 * pixel x matching right column x - d (SpatialTransformer_grid's convention):
 *   valid    lo <= d < hi; a NaN is not valid
 *   target   t = rintf(float(x) - d) in fp32, half to even (np.round, torch.round); x LANDS if it is valid and 0 <= t < W.  -0.5 rounds
 *            to -0 and lands in column 0; W - 0.5 rounds to W, outside the row, only for an even W
 *   owner    of right column r: the LARGEST x that lands on r, -1 if none -- the last writer of a raster-order loop and, the pixel
 *            further right having the larger disparity up to the rounding step, the surface nearer the sensor
 *   right_disparity[r] = d[owner], else fill_disparity;  right_label[r] = float(label[owner]), else fill_label;
 *   left_visible[x]    = lands(x) and owner[t(x)] == x, one byte 0 / 1
 * No value is interpolated: every output is a selection, so the PyTorch composition gives the same bits.  One workgroup per row; the
 * owners are an integer maximum in LDS (order-independent: two calls give the same bits), no floating-point atomics.  label: label_dtype
 * 0 = int64, 1 = uint8, 2 = float32, pixel (b, h, x) at b * label_image_stride + h * label_row_stride + x elements.  Any output may be
 * NULL and is then skipped, at least one is required; label is NULL exactly when right_label is.  lo >= hi or a NaN range: -1.
 * W > 8192 (32 KB of owners), 2^31 or more elements, 2^31 or more rows: -2. */
int ss_right_view_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                      long long label_image_stride, int B, int H, int W, float lo, float hi, float fill_disparity, float fill_label,
                      float* right_disparity, float* right_label, unsigned char* left_visible, ss_stream_t stream);
/* Left-right consistency of two estimates in the convention above: disp_right[r] is the disparity of RIGHT pixel r (its left match at
 * r + disp_right[r]) -- the form right_disparity has, and minus what the model returns for the swapped pair.
 *   diff[x] = |disp_left[x] - disp_right[t(x)]| in fp32 where x lands and disp_right[t(x)] is valid, +inf elsewhere
 *   consistent[x] = diff[x] <= threshold, one byte 0 / 1
 * consistent or diff may be NULL, not both.  A negative or NaN threshold, lo >= hi or a NaN range: -1.  2^31 or more elements: -2. */
int ss_lr_consistency_fwd(const float* disp_left, const float* disp_right, int B, int H, int W, float lo, float hi, float threshold,
                          unsigned char* consistent, float* diff, ss_stream_t stream);
/* ---- disparity refinement: the left-right check and the semantic hole fill, csrc/disparity_refine.hip ----
 * The post-processing of a stereo result, with what a generic fill lacks: a hole takes its value from the surface it belongs to.  The
 * reference has no such step; these are this project's definitions.  Row-wise, per image and row: d the LEFT view's float32 disparity,
 * dR an optional right-view disparity in the form right_disparity has (-model(right, left) for a model), keep an optional byte mask,
 * label an optional label map (label_dtype and strides as ss_right_view_fwd reads them), (lo, hi) the valid range.
 *   in range       lo <= v < hi; a NaN is not
 *   consistent[x]  ss_lr_consistency_fwd's, by the same device function; defined only with dR
 *   source[x]      in_range(d[x]) and (no keep or keep[x] != 0) and (no dR or consistent[x])
 *   class[x]       int(v) where the label value v is integer-valued and 0 <= v < 8; NONE for every other value (negative, 8 or more,
 *                  a fraction, NaN) and without a label.  US3D's ignored class 5 is an ordinary class here.
 *   candidates     of a pixel x that is no source, with max_gap >= 1:
 *                  tier 1, only if class[x] is not NONE: L = the largest x' < x with source[x'] and class[x'] == class[x], R = the
 *                  smallest such x' > x; each is dropped if |x - x'| > max_gap (the nearest is the only candidate of its side)
 *                  tier 2, if tier 1 gave no candidate and `fallback` is set: the same without the class condition (sources of class
 *                  NONE serve it too)
 *   choice         one side alone wins.  Both, prefer = 0 ("background"): R wins iff d[R] < d[L], or d[R] == d[L] and R - x < x - L --
 *                  the smaller disparity is the surface further from the sensor; prefer = 1 ("nearest"): R wins iff R - x < x - L, or
 *                  the distances are equal and d[R] < d[L].  Otherwise L wins.  Plain fp32 comparisons: -0.0 == 0.0.
 *   out_disparity  d[x] bit for bit on a source, d[x*] of the chosen candidate x* on a filled pixel, fill_value elsewhere
 *   kind           one byte: 0 kept, 1 filled from the same class, 2 filled from any class, 3 unfilled
 *   source         int32: x on a kept pixel, x* on a filled one, -1 on an unfilled one
 *   consistent     one byte 0 / 1
 * Nothing is interpolated: every output is a selection, one subtraction or a comparison, so the PyTorch composition gives the same
 * bits.  One workgroup per row: a byte per pixel in LDS, the last / first source column per class carried across the row by an exclusive
 * integer maximum / minimum scan over the threads; two calls give the same bits.  Any output may be NULL and is then
 * skipped, at least one is required; consistent needs disparity_right.  lo >= hi or a NaN range, with disparity_right a negative or NaN
 * threshold, max_gap < 1, prefer or fallback outside {0, 1}, label strides that leave the tensor: -1.  W > 8192 (9 bytes of LDS per
 * column), 2^31 or more elements, 2^31 or more rows: -2. */
int ss_disparity_refine_fwd(const float* disparity, const float* disparity_right, const unsigned char* keep, const void* label,
                            int label_dtype, long long label_row_stride, long long label_image_stride, int B, int H, int W, float lo,
                            float hi, float threshold, int max_gap, int prefer, int fallback, float fill_value, float* out_disparity,
                            unsigned char* kind, int* source, unsigned char* consistent, ss_stream_t stream);
/* ---- disparity refinement: fill along rows and columns, csrc/disparity_fill2d.hip ----
 * The same fill looking in four directions, as SGM and MC-CNN fill occlusions: a hole whose own surface continues directly above or
 * below it need not be filled from max_gap columns away, or from another class, and a row without any source is no longer lost.  `in
 * range`, `consistent`, `source`, `class`, the tiers, `kind` and `out_disparity` are those of the section "disparity refinement",
 * unchanged.  What changes, per image, with max_gap_x >= 1 and max_gap_y >= 1:
 *   candidates     of a pixel (y, x) that is no source.  Tier 1, only if class[y,x] is not NONE: L / R = the nearest source of its
 *                  class in its ROW to the left / right, exactly as above; U / D = the nearest source of its class in its COLUMN above
 *                  (y' < y) / below (y' > y).  L, R are dropped if |x - x'| > max_gap_x; U, D if |y - y'| > max_gap_y.  Tier 2, if
 *                  tier 1 gave no candidate and `fallback` is set: the same without the class condition
 *   choice         the candidates in the order L, R, U, D, each with its value v = d at the candidate and its distance g (columns or
 *                  rows).  prefer = 0 ("background") takes the least (v, g, order), prefer = 1 ("nearest") the least (g, v, order):
 *                  tuples compared lexicographically, v by plain fp32 comparisons (-0.0 == 0.0; no source is a NaN).  With only L
 *                  and R present this is the row fill's rule word for word: R wins iff d[R] < d[L], or the values are equal and R is
 *                  nearer ("nearest": iff R is nearer, or equally far and smaller), otherwise L
 *   out_disparity  d[y,x] bit for bit on a source, d at the chosen candidate (y*, x*) on a filled pixel, fill_value elsewhere
 *   kind           one byte: 0 kept, 1 filled from the same class, 2 filled from any class, 3 unfilled
 *   source         int32: the column x* of the chosen pixel; x on a kept pixel, -1 on an unfilled one
 *   source_row     int32: its row y*; y on a kept pixel, -1 on an unfilled one
 *   consistent     one byte 0 / 1, as above
 * Nothing is interpolated: every output is a selection or a comparison, so the kernels, the PyTorch composition and a sequential
 * restatement agree bit for bit, and two calls give the same bits.  Four launches on the caller's stream over tiles of 64 rows x 256
 * columns: the byte of every pixel and per tile and column the last / first source row of every class; an exclusive scan of those
 * summaries over the at most 128 tiles of a column; a sweep down and up every tile that writes each pixel's U and D as 16-bit rows
 * (0xFFFF for none); and one workgroup per row that runs the row fill's own scans and makes the choice.  No launch waits on another
 * workgroup, no atomics, nothing comes back to the host.
 * scratch: ss_disparity_fill2d_scratch(B, H, W) bytes, 16-byte aligned; every byte that is read is written by the same call first.
 * Each output may be NULL and is then skipped, at least one is required; consistent needs disparity_right.  A NULL disparity or
 * scratch, all outputs NULL, consistent without disparity_right, lo >= hi or a NaN range, with disparity_right a negative or NaN
 * threshold, a gap < 1, prefer or fallback outside {0, 1}, a bad label_dtype, label strides that leave the tensor, non-positive B, H
 * or W, a scratch that is too small or not 16-byte aligned: -1.  W > 8192 or H > 8192 (rows and columns travel as 16-bit values),
 * 2^31 or more elements: -2.  All of it is checked before any launch. */
int ss_disparity_fill2d_scratch(int B, int H, int W, long long* bytes);
int ss_disparity_fill2d_fwd(const float* disparity, const float* disparity_right, const unsigned char* keep, const void* label,
                            int label_dtype, long long label_row_stride, long long label_image_stride, int B, int H, int W, float lo,
                            float hi, float threshold, int max_gap_x, int max_gap_y, int prefer, int fallback, float fill_value,
                            void* scratch, long long scratch_bytes, float* out_disparity, unsigned char* kind, int* source,
                            int* source_row, unsigned char* consistent, ss_stream_t stream);
/* ---- disparity refinement: class-aware median, csrc/disparity_median.hip ----
 * What follows the row fill: a 2-D median that removes what a row-wise fill leaves (streaks where neighbouring rows chose different
 * sources, isolated outliers, rows without any source) and keeps the steps between surfaces sharp, because a pixel is smoothed only
 * with pixels of its own predicted class.  The reference has no such step; these are this project's definitions.  Per image: d a
 * float32 disparity map [B,H,W], label an optional label map (label_dtype and strides as ss_right_view_fwd reads them), where an
 * optional byte mask, (lo, hi) the valid range, r = radius.
 *   valid(v)       lo <= v < hi; a NaN is not valid
 *   class          as above: int(v) for an integer-valued label 0 <= v < 8; NONE for every other value and without a label
 *   window         of (y, x): the pixels (y', x') of the same image with |y - y'| <= r and |x - x'| <= r that lie inside the image.
 *                  Nothing is padded: border windows are smaller
 *   members        the valid pixels of the window; with same_class set and class[y,x] != NONE only those whose class equals the
 *                  centre's.  A centre of class NONE takes all valid pixels.  The centre is a member if it is valid.  n: their number
 *   order          the total order of the fp32 bit patterns by the monotone integer key k = b ^ ((b >> 31) & 0x7fffffff), b the value's
 *                  bits as a signed 32-bit integer, compared as signed integers: -0.0 < +0.0, and the result does not depend on how
 *                  ties are visited.  No member is a NaN, and neither INT32_MIN nor INT32_MAX is the key of a valid value
 *   pick           the lower median: the member at index (n - 1) / 2 of the ascending order
 *   target         (where is absent or where[y,x] != 0) and (valid(d[y,x]) or fill_holes) and n >= max(1, min_count)
 *   out_disparity  the pick, bit for bit, on a target; d[y,x] bit for bit on every other pixel (a NaN or a -999 passes through)
 *   count          one byte: n on a target, 0 elsewhere
 * Nothing is interpolated: every output is a selection, so the PyTorch composition gives the same bits.  One workgroup per tile of
 * 16 x 64 pixels, the tile and its halo as keys in LDS, a fixed compare-exchange network per pixel (non-members enter as alternating
 * INT32_MIN / INT32_MAX sentinels, so the middle of all (2r + 1)^2 slots is the lower median of the members); two calls give the same
 * bits.  count may be NULL, out_disparity may not.  A NULL disparity or out_disparity, out_disparity == disparity (neighbours are read
 * after a pixel could be written: in place is refused), lo >= hi or a NaN range, radius < 1, same_class or fill_holes outside {0, 1},
 * min_count < 1 or > (2r + 1)^2, a bad label_dtype, label strides that leave the tensor, non-positive B, H or W: -1.  radius > 2,
 * 2^31 or more elements: -2. */
int ss_disparity_median_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                            long long label_image_stride, const unsigned char* where, int B, int H, int W, float lo, float hi,
                            int radius, int same_class, int fill_holes, int min_count, float* out_disparity,
                            unsigned char* count, ss_stream_t stream);
/* ---- disparity refinement: speckle removal, csrc/disparity_speckle.hip ----
 * What comes before the row fill: small connected blobs of wrong disparity (a mismatched roof patch, a tree crown, a moving car) pass
 * the left-right check, would serve the fill as sources and are larger than half a median window.  They are found by connected-
 * component labelling and removed.  The reference has no such step and OpenCV's filterSpeckles knows no classes; these are this
 * project's definitions.  Per image: d a float32 disparity map [B,H,W], label an optional label map (label_dtype and strides as
 * ss_right_view_fwd reads them), where an optional byte mask, (lo, hi) the valid range, max_diff a float32 >= 0, max_size an
 * integer >= 0.
 *   valid(v)       lo <= v < hi; a NaN is not valid (the median's definition)
 *   class          as above: int(v) for an integer-valued label 0 <= v < 8; NONE for every other value and without a label
 *   link(p, q)     of two 4-neighbours (left / right, up / down) of the same image: both are valid, and
 *                  fabsf(d[p] - d[q]) <= max_diff with ONE fp32 subtraction, rounded once (a NaN difference links nothing), and --
 *                  with same_class set -- class[p] == class[q], NONE being equal to NONE.  Diagonals never link; nothing links
 *                  across the images of a batch
 *   component      the relation is symmetric; a component is a class of its transitive closure: a chain 0, 1, 2, 3 ... with
 *                  max_diff = 1 is ONE component, as in OpenCV
 *   component[p]   int32: the smallest linear index y * W + x among the pixels of p's component; -1 on a pixel that is not valid
 *   size[p]        int32: the number of pixels of p's component; 0 on a pixel that is not valid
 *   speckle[p]     one byte 0 / 1: valid(d[p]) and size[p] <= max_size and (where is absent or where[p] != 0)
 *   out_disparity  fill_value on a speckle; d[p] bit for bit on every other pixel (a NaN or a -999 passes through)
 * component and size are integers fixed by these definitions, whatever order the unions ran in: the kernel, the PyTorch composition
 * and a sequential flood fill agree exactly, and two calls give the same bits.  Union-find with the smallest index as the root, four
 * launches on the caller's stream: one workgroup per tile of 32 x 64 pixels labels its tile in LDS; one thread per linked pixel pair
 * across a tile boundary unites the two in global memory (agent-scope integer atomicMin, every decision on the value it returned);
 * every tile-local root adds its count to its final root (integer atomicAdd: one per local root, not one per pixel); one pass per
 * pixel writes the outputs.  No launch waits on another workgroup, no floating-point atomics, nothing comes back to the host.
 * scratch: ss_disparity_speckle_scratch(B, H, W) bytes (two int32 planes), 16-byte aligned, wholly overwritten by every call.
 * Each output may be NULL and is then skipped, at least one is required.  The last pass reads nothing of the disparity but d[p] for
 * p: out_disparity == disparity (in place) is ALLOWED.  A NULL disparity or scratch, all outputs NULL, lo >= hi or a NaN range, a
 * negative or NaN max_diff, max_size < 0, same_class outside {0, 1}, a bad label_dtype, label strides that leave the tensor,
 * non-positive B, H or W, a scratch that is too small or not 16-byte aligned: -1.  2^31 or more elements: -2. */
int ss_disparity_speckle_scratch(int B, int H, int W, long long* bytes);
int ss_disparity_speckle_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                             long long label_image_stride, const unsigned char* where, int B, int H, int W, float lo, float hi,
                             float max_diff, int max_size, int same_class, float fill_value, void* scratch, long long scratch_bytes,
                             float* out_disparity, unsigned char* out_speckle, int* out_size, int* out_component, ss_stream_t stream);
/* ---- scene inference: tile windows and the feathered mosaic, csrc/scene_tiles.hip ----
 * What stands around the model call when the input is a scene and not a tile.  The reference has nothing of the kind (its evaluation
 * loader carries top_pad / right_pad keys that are always 0).
 *   window   tile i of th x tw pixels at origin (oy, ox), anywhere: it may overhang the scene
 *   weights  per axis w(i) = min(i + 1, T - i, R) for window-local index i, tile size T and ramp R: integers, never below 1; a tile
 *            pixel weighs float(wy(iy)) * float(wx(ix))
 *   blend    per mosaic pixel over the covering RESIDENT tiles in ascending (ty, tx): num = num + w * v, den = den + w, every product
 *            and sum rounded to fp32, out = num / den with one IEEE division; under ONE tile out = v, the tile's own value (not
 *            (w * v) / w, which rounds twice)
 * ss_tile_views_fwd cuts the windows of a scene pair and applies ToTensor + Normalize in the same pass: left, right uint8 [H,W,3],
 * origins int32 [n][2] as (y, x) in DEVICE memory, table as ss_prep_views_fwd takes it -> out_left, out_right float32 [n,3,th,tw],
 * out[i][c][y][x] = table[c][scene[oy + y][ox + x][c]] inside the scene and 0.0f off it (the mean colour in normalised space).  right
 * and out_right may both be NULL (one view).  n, th, tw, H or W <= 0: -1.  A tensor of 2^31 or more elements: -2. */
int ss_tile_views_fwd(const unsigned char* left, const unsigned char* right, const int* origins, const float* table, int n, int th,
                      int tw, int H, int W, float* out_left, float* out_right, ss_stream_t stream);
/* Gathers finished tiles into rows y0 <= y < y1 of the mosaic; no other row is written.  disp_tiles, logit_tiles: DEVICE tables of
 * nty * ntx addresses, tile (ty, tx) at ty * ntx + tx: its disparity float32 [th,tw] and its logits float32 [C,th,tw], read in place
 * (a batch of tiles is data_ptr() + b * stride); entry 0 = not resident, the tile is skipped.  origin_y [nty], origin_x [ntx]: int32
 * in DEVICE memory, ascending.  ry, rx: the ramps.  Per pixel, with the blend above:
 *   disparity [H,W]    num / den of the tiles' disparities
 *   logits    [C,H,W]  the same per channel
 *   label     [H,W]    uint8, the lowest index of the largest blended logit (np.argmax's rule; a NaN counts as the maximum)
 *   spread    [H,W]    max - min of the covering tiles' disparities: 0 under one tile, the seam diagnostic
 *   count     [H,W]    uint8, the number of covering tiles
 * Any output may be NULL and is then skipped, at least one is required; logits and label need logit_tiles, which is NULL exactly when
 * C is 0.  The order is fixed and nothing is atomic: two calls give the same bits.  Every tile pixel is read once.  A pixel of the
 * range that no resident tile covers gets 0 / 0.  A NULL required pointer, th or tw <= 0, ry or rx < 1, y0 > y1 or a range outside
 * [0, H]: -1.  C > 8, more than 256 windows on an axis, 2^31 or more elements in a tile or in an output: -2. */
int ss_tile_blend_fwd(const long long* disp_tiles, const long long* logit_tiles, const int* origin_y, const int* origin_x, int nty,
                      int ntx, int th, int tw, int C, int ry, int rx, int H, int W, int y0, int y1, float* disparity, float* logits,
                      unsigned char* label, float* spread, unsigned char* count, ss_stream_t stream);
/* ---- training augmentation, csrc/augment.hip ----
 * The reference's KITTI recipe (datasets/kitti_dataset_15_aug.py:100-156) from the raw arrays on the device, plus a vertical flip and a
 * horizontal flip with the views swapped.  left, right uint8 [B,H,W,3]; the outputs are th x tw crops.  All photometric steps work on
 * uint8 values, each stage rounded as PIL rounds it; u is a channel value of the source view that feeds OUTPUT view v of an item:
 *   luma    (19595 r + 38470 g + 7471 b + 0x8000) >> 16
 *   blend   blend(deg, x, f) = trunc(clamp(float(deg) + f * float(x - deg), 0, 255)) in fp32, the product rounded before the sum
 *   T1      brightness then gamma: T1[u] = G[blend(0, u, b)], a 256-entry table per (item, output view) that the CALLER builds
 *   m       int(S / N + 0.5) in double, S the exact sum of luma(T1[r], T1[g], T1[b]) over the WHOLE source image, N = H W
 *   u3, u4  u3 = blend(m, T1[u], contrast);  u4[ch] = blend(luma(u3), u3[ch], saturation)
 *   source  output pixel (y, x) reads row y0 + (vflip ? th - 1 - y : y) and column x0 + x; with the swap the image is mirrored and
 *           the views exchanged before the crop: column W - 1 - (x0 + x) of the OTHER view, and the maps are right_disparity /
 *           right_label (ss_right_view_fwd of the full items), mirrored the same way
 *   occluder  on the output right view of a flagged item: crop pixels inside [cy - sy, cy + sy) x [cx - sx, cx + sx) (rows first,
 *           clipped to the crop) take floor(Sc / (th tw)) per channel, Sc the exact sum of u4 over the crop of that view
 *   views   out[b][ch][y][x] = table[ch][u4], table as ss_prep_views_fwd takes it
 *   maps    the selected pixels: a disparity as float(v) * disp_scale (a swapped item: right_disparity as it is), a label widened to
 *           float32; level k at (y, x) is the augmented full-resolution map at (y k, x k)
 * The parameter block, DEVICE memory, little-endian, one record of 560 bytes per item:
 *   offset  0  int32  y0, x0                     the crop's origin
 *           8  int32  flags                      bit 0 vflip, bit 1 swap, bit 2 occluder
 *          12  int32  cy, sy, cx, sx             the occluder in crop coordinates
 *          28  int32  reserved
 *          32  float  contrast[2]                per OUTPUT view (0 left, 1 right)
 *          40  float  saturation[2]
 *          48  uint8  T1[2][256]
 * No entry point can read the block: the kernels clamp the origin into [0, H - th] x [0, W - tw] and the rectangle into the crop, so a
 * wrong block gives wrong pixels, never an address outside the tensors.
 * Three launches on one stream, in this order: ss_augment_stats_fwd (64-bit integer partial sums of the luma, per workgroup),
 * ss_augment_occluder_fwd (only when an item has an occluder: integer partial channel sums of u4) and ss_augment_write_fwd, which adds
 * the partials -- integers, exact in any order: two calls give the same bits -- builds the tables in LDS and writes every non-NULL
 * output in one pass that reads only the pixels it samples.  No atomics, no finish launch.  Nothing comes back to the host.
 * NULL or non-positive arguments, th > H, tw > W, a workspace that is too small or not 8-byte aligned: -1.  2^31 or more elements in a
 * view, more than 65535 items, levels with th or tw not divisible by 16: -2. */
int ss_augment_param_bytes(int B, long long* bytes);
int ss_augment_scratch_bytes(int B, int H, int W, int th, int tw, long long* bytes);
int ss_augment_stats_fwd(const unsigned char* left, const unsigned char* right, const void* params, int B, int H, int W, int th, int tw,
                         void* workspace, long long workspace_bytes, ss_stream_t stream);
int ss_augment_occluder_fwd(const unsigned char* left, const unsigned char* right, const void* params, int B, int H, int W, int th,
                            int tw, void* workspace, long long workspace_bytes, ss_stream_t stream);
/* have_occluder: 1 when ss_augment_occluder_fwd ran for this block, 0 = the occluder flags are ignored.  disparity (disp_dtype 0 =
 * float32, 1 = int32) and label (label_dtype and strides as ss_right_view_fwd reads them) may be NULL when none of their outputs is asked
 * for; right_disparity / right_label float32 [B,H,W] are read for swapped items only and may be NULL when no item swaps (a swapped item
 * without them gets -999 / 5).  Outputs: out_left, out_right [B,3,th,tw]; disparity_out, label_out [B,th,tw]; disparity_k, label_k
 * [B,th/k,tw/k].  A NULL output is skipped, at least one is required. */
int ss_augment_write_fwd(const unsigned char* left, const unsigned char* right, const void* params, const float* table,
                         const void* disparity, int disp_dtype, float disp_scale, const void* label, int label_dtype,
                         long long label_row_stride, long long label_image_stride, const float* right_disparity,
                         const float* right_label, int B, int H, int W, int th, int tw, const void* workspace,
                         long long workspace_bytes, int have_occluder, float* out_left, float* out_right, float* disparity_out,
                         float* disparity_4, float* disparity_8, float* disparity_16, float* label_out, float* label_2, float* label_4,
                         ss_stream_t stream);
/* Measurement aid (bench.py): a plain device copy, 16 bytes per lane, nontemporal -- the HBM rate a streaming kernel can
 * reach on this box, which SURVEY.md section 8(d) asks the bandwidth fractions to be read against.  bytes % 16 == 0. */
int ss_tool_copy_fwd(const void* src, void* dst, long long bytes, ss_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMSTEREO_HIP_H */
