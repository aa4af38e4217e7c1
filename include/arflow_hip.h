/*
 * arflow_hip.h -- C ABI of libarflow_hip.so: the MI355X (gfx950) kernels for the ARFlow hot path
 * (cost-volume correlation, bilinear warp, forward-splat occlusion maps, census / SSIM / L1
 * photometric terms, edge-aware smoothness).
 *
 * Drop-in boundary.  The reference's only native boundary for this path is the pybind11 module
 * `correlation_cuda` (models/correlation_package/correlation_cuda.cc:169-172) with
 *     int forward (Tensor& input1, Tensor& input2, Tensor& rInput1, Tensor& rInput2, Tensor& output,
 *                  int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
 *                  int corr_type_multiply)                                  (correlation_cuda.cc:10-16)
 *     int backward(input1, input2, rInput1, rInput2, gradOutput, gradInput1, gradInput2, ...6 ints)
 *                                                                          (correlation_cuda.cc:89-96)
 * arflow_corr_fwd / arflow_corr_bwd replace those two entry points.  Every other function below
 * replaces a pure-PyTorch function of the reference (cited per function); the Python mirror in
 * arflow_amd/ binds them with ctypes (see INTEGRATION.md for the reference-side stub).
 *
 * Conventions (all functions):
 *   - plain pointers to DEVICE memory, fp32, NCHW, contiguous unless a stride argument says otherwise;
 *   - outputs are caller-allocated; outputs that are accumulated into (scatter targets, reduction
 *     sums) are zero-filled by the callee on the same stream (the reference's callee zero-fills too,
 *     correlation_cuda.cc:40-42,112-115);
 *   - `stream` is a hipStream_t (NULL = default stream); the call only enqueues work: no
 *     synchronisation, no allocation, no global state -> re-entrant per stream, capturable in a
 *     hipGraph;
 *   - return 0 on success, ARFLOW_E* (< 0) for argument errors, -(int)hipError_t - 2000 when the
 *     launch failed (the reference returns 0/1 and raises "CUDA call failed",
 *     correlation_cuda.cc:81-83);  arflow_strerror() names a code.
 */
#ifndef ARFLOW_HIP_H
#define ARFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* arflow_stream_t; /* hipStream_t */

#define ARFLOW_OK 0
#define ARFLOW_ENULL (-1001)   /* required pointer is NULL */
#define ARFLOW_ESHAPE (-1002)  /* non-positive or inconsistent dimension */
#define ARFLOW_EPARAM (-1003)  /* unsupported mode / parameter value */
#define ARFLOW_ENONDET (-1004) /* deterministic mode is on and this operation only has an atomic form */
#define ARFLOW_ELAUNCH_BASE (-2000)

#define ARFLOW_PAD_ZEROS 0
#define ARFLOW_PAD_BORDER 1

/* how flow is turned into grid_sample coordinates */
#define ARFLOW_NORM_ARFLOW 0 /* utils/warp_utils.py:16-23,83-90: 2*(x+u)/(W-1)-1, un-normalised per align_corners */
#define ARFLOW_NORM_UFLOW 1  /* utils/uflow_utils.py:53-77: 2*(x+u)/max(W-1,1)-1, align_corners=True */
#define ARFLOW_NORM_UFLOW_ABS 2 /* same, but the "flow" argument already holds absolute coordinates
                                   (resample(source, coords) with coords = flow_to_warp(flow)) */
#define ARFLOW_COORDS_ABS 2     /* OR into `variant` / `mode` of splat_map / coord_mask: input holds
                                   absolute coordinates instead of a flow */

/* Reduction outputs ("sums") are NOT single scalars: every workgroup of a reduction kernel STORES its partial sums into
 * its own row of ARFLOW_SUM_COLS floats and zero-fills the rows beyond the kernel's grid -- no zero-fill launch, no
 * atomics, and a value that does not depend on the order the workgroups finish in.  A `sums` argument points to
 * arflow_sums_rows(B, H, W) * ARFLOW_SUM_COLS floats (need not be initialised; every row is written by the call);
 * quantity k is  sum over all rows r of  sums[r * ARFLOW_SUM_COLS + k]. */
#define ARFLOW_SUM_COLS 4
int arflow_sums_rows(int B, int H, int W);

int arflow_abi_version(void);
const char* arflow_strerror(int code);

/* ---- deterministic mode ------------------------------------------------------------------------
 * One process-wide switch (initial value: environment variable ARFLOW_DETERMINISTIC=1, else off).  While it is on, every
 * entry point whose default kernels end in floating-point atomics -- the source gradient of arflow_warp_bwd[_bf16] and of
 * arflow_level_bwd, their channel-split flow gradient, arflow_splat_map / arflow_splat_smooth_fwd, the bias gradient of
 * arflow_bias_act_bwd -- launches fixed-order kernels instead: each output element is the sum of its terms in ascending
 * (target pixel, tap) order, a function of the data indices alone, so two calls on the same inputs agree bit for bit.
 * The switch selects kernels at launch; default-mode kernels and results are untouched.  Entry points that only have
 * an atomic form (arflow_corr_general_bwd, arflow_warp_nearest_bwd, arflow_warp_bicubic_bwd with gsrc) return
 * ARFLOW_ENONDET while it is on.  arflow_level_bwd_ws_bytes honours the mode: size the workspace under the mode the call
 * will run in.  set returns the previous value.  [No reference counterpart.] */
int arflow_set_deterministic(int on);
int arflow_get_deterministic(void);

/* out[b,c] = factor * upsample_bilinear2d(flow[b,c], scale_factor = factor) in ATen's arithmetic, i.e.
 * F.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners) of models/pwclite.py:54,66,92,104,
 * models/pwclite_uflow.py:104,124 and utils/uflow_utils.py:163-180 upsample(is_flow) in one launch; factor 2 or 4 (else
 * ARFLOW_EPARAM).  flow: [B,2,h,w] contiguous -> out: [B,2,factor*h,factor*w].  arflow_flow_up_bwd is its adjoint as a GATHER:
 * one thread per coarse cell adds the fine pixels that read it, rows then columns ascending -- every element of gcoarse
 * [B,2,h,w] written, no atomics, bitwise reproducible (ATen's backward scatters with atomics). */
int arflow_flow_up_fwd(const float* flow, float* out, int B, int h, int w, int factor, int align_corners,
                       arflow_stream_t stream);
int arflow_flow_up_bwd(const float* gfine, float* gcoarse, int B, int h, int w, int factor, int align_corners,
                       arflow_stream_t stream);
/* Output upsample of the probabilistic PWC model (models/uflow_prob_model.py:223-250 upsample_out) over all channels in one
 * launch: out[b,c] = s_c * upsample_bilinear2d(in[b,c] + b_c, x2, align_corners=False) with s_c = 2 for c < n_flow (else 1)
 * and b_c = diag_bias for n_flow <= c < n_flow + n_diag (else 0); the bias is added on load, before the blend.  fp32, planes
 * contiguous (h*w floats between channels); every tensor has its own batch stride in floats (>= C * plane when B > 1), so
 * `in` can be a channel slice of a wider tensor and `out` a slot of a concatenated buffer.  in: [B,C,h,w] -> out:
 * [B,C,2h,2w].  One float4 store per lane where w is even and out / out_bstride are 16-byte aligned, else a scalar path.
 * arflow_out_up2_bwd is the adjoint as a GATHER (gfine [B,C,2h,2w] -> gcoarse [B,C,h,w]): one coarse cell adds the <= 4x4
 * fine pixels that read it, rows then columns ascending; every element of gcoarse written, no atomics, bitwise
 * reproducible.  arflow_out_tail_fwd applies the rule twice in one launch -- out1 [B,C,2h,2w] and out0 [B,C,4h,4w], both
 * contiguous, from one read of `in` -- and is bitwise equal to two arflow_out_up2_fwd launches (its adjoint is two
 * arflow_out_up2_bwd launches). */
int arflow_out_up2_fwd(const float* in, long in_bstride, float* out, long out_bstride, int B, int C, int h, int w, int n_flow,
                       int n_diag, float diag_bias, arflow_stream_t stream);
int arflow_out_up2_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C, int h,
                       int w, int n_flow, arflow_stream_t stream);
int arflow_out_tail_fwd(const float* in, long in_bstride, float* out1, float* out0, int B, int C, int h, int w, int n_flow,
                        int n_diag, float diag_bias, arflow_stream_t stream);
/* The align_corners=True sibling of arflow_out_up2_* for factor 2 or 4 (else ARFLOW_EPARAM), the upsample of the (flow,
 * log-variance) state of models/pwclite_prob.py:183-186,216-217: out[b,c] = s_c * upsample_bilinear2d(in[b,c] + b_c, x factor,
 * align_corners=True) with s_c = factor for c < n_flow (else 1) and b_c = diag_bias for n_flow <= c < n_flow + n_diag (else 0),
 * the bias added on load.  Source coordinate and weights in ATen's fp32 order: scale = (h - 1) / (H - 1), src = scale * dst,
 * floor, lambda and 1 - lambda.  Layout rules, slices and batch strides as arflow_out_up2_fwd; in [B,C,h,w] -> out
 * [B,C,factor h,factor w]; float4 stores where factor * w % 4 == 0 and out / out_bstride are 16-byte aligned.  h, w <= 2048.
 * arflow_prob_up_bwd is the adjoint as a GATHER (gfine [B,C,factor h,factor w] -> gcoarse [B,C,h,w]): one coarse cell adds
 * the fine pixels that read it, rows then columns ascending; every element written, no atomics, bitwise reproducible. */
int arflow_prob_up_fwd(const float* in, long in_bstride, float* out, long out_bstride, int B, int C, int h, int w, int factor,
                       int n_flow, int n_diag, float diag_bias, arflow_stream_t stream);
int arflow_prob_up_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C, int h,
                       int w, int factor, int n_flow, arflow_stream_t stream);
/* HIP keeps ONE "last error" per host thread.  If a code was already pending when an entry point is entered
 * (left by the host framework or an unchecked earlier call) it is not attributed to this library's launch and
 * not dropped either: the first such hipError_t is kept (and reported once on stderr) until the host reads it
 * here.  Returns that hipError_t (0 = none) and clears the slot.  [No reference counterpart: the reference
 * checks cudaGetLastError() once after its launches, correlation_cuda_kernel.cu:383-392.] */
int arflow_take_stale_error(void);
/* Profiling aid: enqueues a one-wave no-op kernel (`af_marker_kernel`) that delimits the dispatches of consecutive calls in
 * a rocprofv3 kernel / counter trace (tools/kbench.py, tools/pmc_calls.py).  [No reference counterpart.] */
int arflow_profile_marker(int tag, arflow_stream_t stream);

/* ---- cost volume ------------------------------------------------------------------------------
 * out[b, i*(2d+1)+j, y, x] = (1/C) sum_c x1[b,c,y,x] * x2[b,c,y+i-d,x+j-d], zero outside.
 * Replaces correlation_cuda.forward (correlation_cuda.cc:10-87), Correlation.forward
 * (models/correlation_native.py:13-23) and compute_cost_volume (models/uflow_model.py:53-92).
 * x1,x2: [B,C,H,W]; out: [B,(2d+1)^2,H,W]; 1 <= max_disp. */
int arflow_corr_fwd(const float* x1, const float* x2, float* out, unsigned* sign_bits, int B, int C, int H,
                    int W, int max_disp, float negative_slope, arflow_stream_t stream);
/* negative_slope: fused LeakyReLU on the cost volume, out = v > 0 ? v : negative_slope * v -- the
 * activation every caller applies right after the correlation (models/pwclite.py:183-184,
 * models/uflow_model.py:180); 1.0f = plain cost volume.
 * sign_bits (nullable): compact record of `v > 0` for the backward, [B, arflow_corr_sign_planes(), H, W]
 * 32-bit words: bit (i % 3) * 9 + j of plane i / 3 belongs to channel i * 9 + j.  Only produced by the
 * max_disp = 4 fast path: asking for it when arflow_corr_sign_planes(C, W, max_disp) == 0 is ARFLOW_EPARAM. */
int arflow_corr_sign_planes(int C, int W, int max_disp); /* 3, or 0 if this shape has no sign_bits */

/* The same with the cost volume at a BATCH STRIDE: out[b] starts at out + b * out_bstride floats (>= (2d+1)^2*H*W,
 * a multiple of 4), channels and rows contiguous inside a sample -- the volume is written straight into channels
 * [k, k+81) of the [B, Ctot, H, W] buffer the caller's decoder reads as its concatenated input
 * (torch.cat([out_corr_relu, x1, flow, ...], 1) at models/pwclite_uflow.py:218-222, models/pwclite.py:187-189,
 * models/uflow_model.py:192-198), so the 81-channel volume is never copied.  Fast path only
 * (arflow_corr_strided_supported() == 1: max_disp 4, W % 4 == 0, C % 4 == 0), else ARFLOW_EPARAM. */
int arflow_corr_strided_supported(int C, int W, int max_disp);
int arflow_corr_fwd_strided(const float* x1, const float* x2, float* out, long out_bstride, unsigned* sign_bits,
                            int B, int C, int H, int W, int max_disp, float negative_slope, arflow_stream_t stream);

/* Gradients of the above (correlation_cuda.backward, correlation_cuda.cc:89-167; kernels
 * correlation_cuda_kernel.cu:116-300).  gx1 / gx2 may be NULL to skip that gradient. */
int arflow_corr_bwd(const float* gout, const float* out, const unsigned* sign_bits, const float* x1,
                    const float* x2, float* gx1, float* gx2, int B, int C, int H, int W, int max_disp,
                    float negative_slope, arflow_stream_t stream);
/* gout (and out, if given) at batch strides: the gradient of the concatenated decoder input is consumed in place. */
int arflow_corr_bwd_strided(const float* gout, long gout_bstride, const float* out, long out_bstride,
                            const unsigned* sign_bits, const float* x1, const float* x2, float* gx1, float* gx2, int B,
                            int C, int H, int W, int max_disp, float negative_slope, arflow_stream_t stream);
/* With negative_slope != 1 the LeakyReLU derivative is selected per element by the forward's sign_bits
 * (12 bytes per pixel instead of re-reading the 324-byte volume) or, when sign_bits is NULL, by the sign
 * of the forward OUTPUT passed as `out` (as torch's in-place leaky_relu backward does; needs
 * negative_slope > 0).  One of the two must be given; with negative_slope == 1 both may be NULL. */

/* ---- feature normalisation in front of the cost volume ------------------------------------------
 * y_i = (x_i - mu) / sqrt(var + 1e-16), one (mu, var) per sample over both tensors:
 *   ARFLOW_FEATNORM_JOINT  normalize_features of models/pwclite_uflow.py:30-38 (moments of the
 *                          channel-concatenated pair, unbiased variance over 2n - 1)
 *   ARFLOW_FEATNORM_AVG    normalize_features of models/uflow_model.py:8-50 as PWCFlow calls it (:167-172):
 *                          per-tensor mean / unbiased variance over (C,H,W), averaged across the two images
 * x1,x2,y1,y2: [B, n] contiguous (n = C*H*W >= 2).  acc: ARFLOW_FEATNORM_ACC_DOUBLES(B) doubles of scratch
 * (need not be initialised: every workgroup of the reduction pass stores its partial sums into its own row).
 * stats: [B,4] floats written by the forward (m1, m2, mu, std) and read by the backward.
 * Backward: gx1 / gx2 (nullable) = gradients w.r.t. x1 / x2 given g1, g2 = gradients w.r.t. y1, y2. */
#define ARFLOW_FEATNORM_JOINT 0
#define ARFLOW_FEATNORM_AVG 1
#define ARFLOW_FEATNORM_ACC_DOUBLES(B) (4 * (2048 + (B)))
int arflow_featnorm_fwd(const float* x1, const float* x2, float* y1, float* y2, double* acc, float* stats,
                        int B, long n, int mode, arflow_stream_t stream);
int arflow_featnorm_bwd(const float* g1, const float* g2, const float* x1, const float* x2,
                        const float* stats, double* acc, float* gx1, float* gx2, int B, long n, int mode,
                        arflow_stream_t stream);

/* ---- pyramid level, fused --------------------------------------------------------------------
 * One level of the PWC decoders in front of its flow estimator,
 *     flow   = interpolate(flow_coarse * 2, x2, bilinear)                 models/pwclite_uflow.py:208
 *     x2w    = flow_warp(x2, flow)  /  resample(x2, flow_to_warp(flow))   models/pwclite_uflow.py:209, uflow_model.py:164
 *     x1n, x2n = normalize_features([x1, x2w])                            models/pwclite_uflow.py:212-213, uflow_model.py:167-172
 *     vol    = LeakyReLU(corr(x1n, x2n))                                  models/pwclite_uflow.py:214-215, uflow_model.py:174-178
 * as TWO launches forward: (1) arflow_level_warp_fwd -- flow upsample + warp + the partial moments of the
 * normalisation (one row of 4 doubles per workgroup: sum x1, sum x1^2, sum x2w, sum x2w^2); at the level without a
 * flow arflow_level_moments takes its place; (2) arflow_level_corr_fwd -- the cost volume of the NORMALISED pair
 * computed from the raw maps (x1 is normalised in registers, the second map's normalisation is an epilogue term),
 * writing the volume, the normalised first map (the decoder concatenates it) and the sign words of the fused LeakyReLU.
 * The normalised second map, the moment / apply passes and the interpolate / mul launches do not exist.
 *
 * acc: 4 * B * arflow_level_acc_rows(B, C, H, W, has_flow) doubles (not initialised by the caller).
 * flow: [B,2,H/2,W/2] with flow_is_coarse (upsampled x2 inside, align flag up_align_corners; flow_up [B,2,H,W] and /
 * or flow_up2 (batch stride flow_up2_bstride) receive it) or [B,2,H,W]; flow_bstride = floats between samples.
 * out / x1n: volume and normalised first map with batch strides (slots of a concatenated buffer); stats: [B,4]
 * (m1, m2, mu, sigma).  Needs the fast-path shapes (arflow_corr_strided_supported). */
/* The level as ONE call per direction (the entry points the host models use; the stage entry points further down
 * remain for callers that keep their own intermediate buffers):
 *   arflow_level_fwd  = [arflow_level_warp_fwd | arflow_level_moments] + arflow_level_corr_fwd, back to back;
 *   arflow_level_bwd  = arflow_level_corr_bwd + the normalisation's backward (gx1n_direct, the gradient the decoder's
 *     concatenation returns for x1n, is added on load) + the warp's backward (gflow_a [batch stride] and gflow_b
 *     [contiguous], further gradients of the upsampled flow, are added on the way out) + the adjoint of the x2 flow
 *     upsample.  gflow: [B,2,H/2,W/2] with flow_is_coarse, else [B,2,H,W]; flow_full: the fine flow the forward
 *     warped with (flow_up of the forward, or the caller's fine flow; NULL at the level without a warp -- then x2w,
 *     gflow*, gflow are ignored and gx2 is the normalisation's second gradient).
 *   workspace: arflow_level_bwd_ws_bytes(B, C, H, W) bytes of scratch, 256-byte aligned; acc as for the stages. */
int arflow_level_supported(int C, int W, int max_disp);
long arflow_level_bwd_ws_bytes(int B, int C, int H, int W);
int arflow_level_fwd(const float* x1, const float* x2, const float* flow, long flow_bstride, int flow_is_coarse,
                     int up_align_corners, float* flow_up, float* flow_up2, long flow_up2_bstride, float* x2w, int norm_mode,
                     float* out, long out_bstride, float* x1n, long x1n_bstride, unsigned* sign_bits, float* stats,
                     double* acc, int B, int C, int H, int W, int max_disp, float negative_slope, int pad_mode,
                     int align_corners, int coord_norm, arflow_stream_t stream);
/* As arflow_level_fwd, with the partial moments of the feature maps taken where the maps were PRODUCED
 * (arflow_bias_act_fwd_mom rows, [B][nrows][2] doubles of (sum, sum of squares)): x1_rows for the first map (the warp launch
 * then does not read it) and, at the level without a warp, x2_rows for the second (no moment pass at all). */
int arflow_level_fwd_m(const float* x1, const float* x2, const float* flow, long flow_bstride, int flow_is_coarse,
                       int up_align_corners, float* flow_up, float* flow_up2, long flow_up2_bstride, float* x2w, int norm_mode,
                       float* out, long out_bstride, float* x1n, long x1n_bstride, unsigned* sign_bits, float* stats,
                       double* acc, const double* x1_rows, int x1_nrows, const double* x2_rows, int x2_nrows, int B, int C, int H,
                       int W, int max_disp, float negative_slope, int pad_mode, int align_corners, int coord_norm,
                       arflow_stream_t stream);
int arflow_level_bwd(const float* gout, long gout_bstride, const unsigned* sign_bits, const float* x1n, long x1n_bstride,
                     const float* gx1n_direct, long gx1n_direct_bstride, const float* x1, const float* x2, const float* x2w,
                     const float* flow_full, long flow_bstride, const float* gflow_a, long gflow_a_bstride,
                     const float* gflow_b, const float* stats, int norm_mode, float* gx1, float* gx2, float* gflow,
                     int flow_is_coarse, int up_align_corners, void* workspace, int B, int C, int H, int W, int max_disp,
                     float negative_slope, int pad_mode, int align_corners, int coord_norm, arflow_stream_t stream);
int arflow_level_acc_rows(int B, int C, int H, int W, int has_flow);
/* Adjoint of the x2 bilinear flow upsample of arflow_level_warp_fwd (flow_up = interpolate(flow * 2, scale 2),
 * models/pwclite.py:178-179, utils/uflow_utils.py:163-180 upsample(is_flow)): gfine [B,2,H,W] -> gcoarse [B,2,H/2,W/2],
 * every element written (no zero-fill needed). */
int arflow_up2_bwd(const float* gfine, float* gcoarse, int B, int H, int W, int up_align_corners, arflow_stream_t stream);
int arflow_level_moments(const float* x1, const float* x2, double* acc, int B, long n, arflow_stream_t stream);
int arflow_level_warp_fwd(const float* x1, const float* x2, const float* flow, long flow_bstride, int flow_is_coarse,
                          int up_align_corners, float* flow_up, float* flow_up2, long flow_up2_bstride, float* x2w,
                          double* acc, int B, int C, int H, int W, int pad_mode, int align_corners, int norm_mode,
                          arflow_stream_t stream);
int arflow_level_corr_fwd(const float* x1, const float* x2w, const double* acc, int acc_rows, int norm_mode, float* out,
                          long out_bstride, float* x1n, long x1n_bstride, unsigned* sign_bits, float* stats, int B, int C,
                          int H, int W, int max_disp, float negative_slope, arflow_stream_t stream);
/* Backward of arflow_level_corr_fwd w.r.t. the NORMALISED maps: gx1n = d/d x1n (correlation part only: the caller adds the
 * gradient the decoder's concatenation returns for x1n), gx2n = d/d x2n; x1n as written by the forward (batch stride),
 * x2w the raw warped map, stats as written by the forward.  The normalisation's own backward is arflow_featnorm_bwd on
 * (gx1n + direct, gx2n, x1, x2w).  sign_bits NULL <=> negative_slope == 1. */
int arflow_level_corr_bwd(const float* gout, long gout_bstride, const unsigned* sign_bits, const float* x1n,
                          long x1n_bstride, const float* x2w, const float* stats, float* gx1n, float* gx2n, int B, int C,
                          int H, int W, int max_disp, float negative_slope, arflow_stream_t stream);

/* ---- conv epilogue of the host models ------------------------------------------------------------
 * y = lrelu(x + bias[c]) for x, y: [B, C, HW] (x == y allowed; bias nullable): the bias add and
 * LeakyReLU(0.1) that follow every convolution of the reference models (models/pwclite.py:10-23,
 * models/uflow_model.py:271-287) in one pass.  Backward: gin = gout * (y > 0 ? 1 : negative_slope) and
 * gbias[c] = sum_{b,hw} gin (gbias nullable, zero-filled here; fp32 atomics -- in deterministic mode one workgroup per
 * channel sums in a fixed order instead). */
int arflow_bias_act_fwd(const float* x, const float* bias, float* y, int B, int C, long HW,
                        float negative_slope, arflow_stream_t stream);
/* As arflow_bias_act_fwd; additionally every workgroup leaves (sum y, sum y^2) of its slice: mom holds
 * [B][arflow_bias_act_mom_rows(C, HW)][2] doubles (every row written by the call) -- the partial moments of
 * normalize_features taken where the feature map is produced (arflow_level_fwd_m consumes them). */
int arflow_bias_act_mom_rows(int C, long HW);
int arflow_bias_act_fwd_mom(const float* x, const float* bias, float* y, double* mom, int B, int C, long HW,
                            float negative_slope, arflow_stream_t stream);
int arflow_bias_act_bwd(const float* gout, const float* y, float* gin, float* gbias, int B, int C, long HW,
                        float negative_slope, arflow_stream_t stream);

/* ---- two-channel 3x3 head convolution ----------------------------------------------------------
 * y = conv2d(x, w, bias) for w: [2, C, 3, 3], stride 1, padding 1, dilation 1, groups 1 -- the flow heads of the
 * reference models (conv_last / predict_flow / the last ContextNetwork conv, models/pwclite.py:48-106, built by
 * conv(..., isReLU=False), models/pwclite.py:10-23), which the vendor library pads into 32-wide tiles.  One pass over
 * x per call, bias folded in; x: [B,C,H,W], y / dy: [B,2,H,W], any B, C, H, W >= 1 (float4 paths when W % 4 == 0 and
 * the pointers are 16-byte aligned).  No atomics anywhere: every result is bitwise reproducible.  All sums are
 * accumulated in double and rounded to fp32 once: the correctly rounded result up to double rounding.
 * bias and dbias are nullable.  The weight gradient leaves per-wave partial sums in `ws`
 * (arflow_headconv_bwd_weight_ws_bytes() bytes, 16-byte aligned, need not be initialised; < 0 = ARFLOW_ESHAPE) and
 * adds them in a second kernel; dbias[o] = sum dy[:, o] comes out of the same pass. */
int arflow_headconv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W,
                        arflow_stream_t stream);
int arflow_headconv_bwd_data(const float* dy, const float* w, float* dx, int B, int C, int H, int W,
                             arflow_stream_t stream);
long arflow_headconv_bwd_weight_ws_bytes(int B, int C, int H, int W);
int arflow_headconv_bwd_weight(const float* x, const float* dy, float* dw, float* dbias, void* ws, int B, int C, int H,
                               int W, arflow_stream_t stream);

/* ---- wide 3x3 convolution on the bf16 matrix cores at fp32 accuracy -----------------------------
 * y[n,k] = sum_c x[n,c] * w[k,c] (cross-correlation as conv2d), 3x3, stride 1, zero padding 1, dilation 1, groups 1, no
 * bias; x: [N,C,H,W], y: [N,K,H,W], packed fp32.  Every fp32 operand is split exactly into three bf16 numbers and six of
 * the nine bf16 products are accumulated, smallest first, in the MFMA's fp32 accumulator: the accuracy of an fp32 FMA chain
 * at 1/6 of the bf16 matrix rate.  The summation order is fixed (no atomics, no split of the reduction): two calls are
 * bitwise equal.
 *
 * arflow_splitconv_pack turns the fp32 weights w: [K,C,3,3] into the three bf16 planes in MFMA fragment order,
 *     packed[plane][tap][K' / 32][C' / 16][lane 64][8],   K' = K padded to 32, C' = C padded to 32, zero in the padding,
 * element j of lane l = W[32 kt + (l & 31)][16 cs + 8 (l >> 5) + j][tap].  transpose_flip = 0 packs W = w;
 * transpose_flip = 1 packs W[c][k][r][s] = w[k][c][2-r][2-s], which makes the data gradient the same convolution:
 * dx = arflow_splitconv_fwd(dy, packed, N, C = K, K = C).  `packed` is 16-byte aligned and holds
 * arflow_splitconv_pack_bytes(K, C) bytes, K and C being the OUTPUT and INPUT channels of the convolution that will read
 * it (for transpose_flip = 1: the weights' C and K); < 0 = ARFLOW_ESHAPE.  Weights change every step: pack per call.
 * ARFLOW_ESHAPE also where N*C*H*W or N*K*H*W exceeds INT_MAX. */
long arflow_splitconv_pack_bytes(int K, int C);
int arflow_splitconv_pack(const float* w, void* packed, int K, int C, int transpose_flip, arflow_stream_t stream);
int arflow_splitconv_fwd(const float* x, const void* packed, float* y, int N, int C, int K, int H, int W,
                         arflow_stream_t stream);

/* arflow_splitconv_fwd with free batch strides and an optional epilogue at the store; arflow_splitconv_fwd is this call with
 * x_bstride = C*H*W, y_bstride = K*H*W, bias = NULL, act = 0.  x: [N,C,H,W] and y: [N,K,H,W] with dense planes, rows and
 * columns and batch strides x_bstride >= C*H*W, y_bstride >= K*H*W floats (else ARFLOW_ESHAPE; also where N*x_bstride or
 * N*y_bstride exceeds INT_MAX): a channel slice of a larger tensor is read, and a channel slot of one written, in place.  The
 * loads and stores are scalar: no alignment beyond 4 bytes is asked of x and y.  PRECONDITION: no element is both read and
 * written.  x and y may be DISJOINT channel ranges of one buffer -- the dense estimator's layer reads x6[:, off:] and writes
 * x6[:, off-K:off] -- but must not overlap.
 * act = 0 stores the sum as arflow_splitconv_fwd does; bias must then be NULL (ARFLOW_EPARAM).  act = 1 stores
 * lrelu(sum + bias[k]) with arflow_bias_act_fwd's arithmetic (v += b; v > 0 ? v : v * negative_slope), b = 0.f for a NULL
 * bias (the add is kept: -0 becomes +0, as in arflow_dense_cat_fwd).  Any other act: ARFLOW_EPARAM.  The sums, their order
 * and so their bits are arflow_splitconv_fwd's. */
int arflow_splitconv_fwd_ex(const float* x, long x_bstride, const void* packed, float* y, long y_bstride, const float* bias,
                            int act, float negative_slope, int N, int C, int K, int H, int W, arflow_stream_t stream);

/* The weight gradient of the same convolution, dw[k,c,r,s] = sum_{n,h,w} dy[n,k,h,w] * x[n,c,h+r-1,w+s-1] (zero outside the
 * image), with the same split of both operands and the same six products; the reduction runs over pixels, which NCHW keeps
 * contiguous per channel, so nothing is transposed.  x: [N,C,H,W] and dy: [N,K,H,W] with dense planes (H*W apart) and batch
 * strides x_bstride >= C*H*W, dy_bstride >= K*H*W floats (else ARFLOW_ESHAPE); dw: [K,C,3,3] packed, every element written
 * (no accumulate-into).  The pixel range is cut into chunks whose partial sums go to `ws`
 * (arflow_splitconv_wgrad_ws_bytes() bytes, 16-byte aligned, need not be initialised; < 0 = ARFLOW_ESHAPE) and are added in
 * ascending order in float64 by a second kernel: fixed order, no atomics, two calls are bitwise equal.  ARFLOW_ESHAPE also
 * where N*C*H*W, N*K*H*W or 9*K*C exceeds INT_MAX; ARFLOW_EPARAM for x, dy or dw off a 4-byte or ws off a 16-byte boundary. */
long arflow_splitconv_wgrad_ws_bytes(int N, int C, int K, int H, int W);
int arflow_splitconv_wgrad(const float* x, long x_bstride, const float* dy, long dy_bstride, float* dw, void* ws, int N, int C,
                           int K, int H, int W, arflow_stream_t stream);

/* ---- phase-mosaic layouts: dilated 3x3 convolutions on the dilation-1 kernels above -------------
 * A 3x3 convolution with dilation d and padding d is d*d independent dilation-1 / padding-1 convolutions on the phases
 * x[:, :, p::d, q::d].  LAYOUT d of a tensor [N,C,H,W] (csrc/phase_plan.hpp) is the dense tensor [Nv,C,Hv,Wv] in which Pg x Qg
 * phase images of Hs = ceil(H/d) x Ws = ceil(W/d) lie side by side with one row / column of zeros between neighbours:
 * Hv = Pg (Hs + 1) - 1, Wv = Qg (Ws + 1) - 1, Nv = N d d / (Pg Qg); real (n, h, w) sits at sample
 * (n (d/Pg) + (h%d)/Pg) (d/Qg) + (w%d)/Qg, row ((h%d)%Pg) (Hs+1) + h/d, column ((w%d)%Qg) (Ws+1) + w/d.  (Pg, Qg) is the pair of
 * divisors of d that costs arflow_splitconv_fwd_ex's pixel tiles the least.  Layout 1 is NCHW.  conv2d(x, w, padding = d,
 * dilation = d) in layout d IS arflow_splitconv_fwd_ex on (Nv, C, Hv, Wv) at the real positions, provided the separators and
 * ragged tails (cells of phases that have a row or column less when d does not divide H or W) of the input hold zero; the
 * outputs there are finite garbage.  The same holds for the data gradient and, with zeros there in dy, the weight gradient.
 *
 * arflow_phase_layout: the host-side plan, out = {Nv, Hv, Wv, Pg, Qg}; needs no GPU.
 * arflow_phase_move: dst (layout d_dst) = src (layout d_src); dst2 != NULL: the same values in layout d_dst2 as well, from the
 *   one read (dst2 == NULL needs d_dst2 == 0 and the reverse, else ARFLOW_EPARAM).  Every separator and tail element of a
 *   destination is stored as zero; those of the source are never loaded.  Every element of every destination is stored.
 * arflow_phase_act_bwd: gin (layout d_b; gin2 in d_b2 likewise) = gout * (y > 0 ? 1 : negative_slope), gout and y in layout d_a:
 *   arflow_bias_act_bwd's arithmetic, zeros at separators and tails.  rows != NULL: [arflow_phase_rows(N, H, W, d_b, d_b2)][C]
 *   float64 partial sums of gin over REAL pixels (by position), one row per workgroup, every row stored; the bias gradient is
 *   their sum, which the caller takes in any fixed order.  No atomics: the same bits in either mode.
 * ARFLOW_ESHAPE: a dimension < 1, d > H or d > W, rows too long for the workgroup's LDS (W beyond about 900), N or C > 65535, or a layout of more than INT_MAX elements --
 * returned before anything is launched.  Sources and destinations must not overlap. */
int arflow_phase_layout(int N, int H, int W, int d, int* nv_hv_wv_pg_qg);
int arflow_phase_rows(int N, int H, int W, int d_dst, int d_dst2);
int arflow_phase_move(const float* src, float* dst, float* dst2, int N, int C, int H, int W, int d_src, int d_dst, int d_dst2,
                      arflow_stream_t stream);
int arflow_phase_act_bwd(const float* gout, const float* y, float* gin, float* gin2, double* rows, int N, int C, int H, int W,
                         int d_a, int d_b, int d_b2, float negative_slope, arflow_stream_t stream);

/* ---- dense flow estimator: concatenating epilogue and gradient gather ---------------------------
 * FlowEstimatorDense (models/pwclite.py:48-66) runs five times x = cat([lrelu(conv(x) + bias), x], 1).
 *
 * arflow_dense_cat_fwd: out[:, :oc] = lrelu(y + bias[c]), out[:, oc:] = x, for y: [B, oc, HW] (the bias-free
 * convolution output), x: [B, C, HW], out: [B, oc + C, HW], all packed; bias nullable.  The arithmetic is
 * arflow_bias_act_fwd's; float4 accesses when HW % 4 == 0 (the pointers must then be 16-byte aligned: ARFLOW_EPARAM).
 *
 * arflow_dense_grad_gather: gy[b, c, :] = d[b, c, :] * (s_0 + s_1 + ... ) for c < oc, with
 *     acc = s_0;  acc = s_1 + acc;  acc = s_2 + acc; ...        (each s_j multiplied by scale_j[b] first, if given)
 * in exactly this nesting and without contraction -- the order autograd accumulates the gradients of a
 * concatenation's slices in -- and d = (act > 0 ? 1 : negative_slope), or 1 when act is NULL.  `srcs` is a HOST array
 * of n_src (1 .. ARFLOW_DENSE_MAX_SRC) descriptors; it travels in the kernel arguments and need not outlive the call.
 * A source's `ptr` addresses channel 0 of the slice in sample 0 (planes of HW floats, dense), `bstride` is its sample
 * stride in floats, `scale` an optional [B] device vector.  act is read in place (sample stride act_bs floats); gy is
 * packed [B, oc, HW].  gbias_rows (nullable): [arflow_dense_gbias_rows(B, HW)][oc] floats, every entry written by
 * the call; the bias gradient is the sum over the rows (fixed order: bitwise reproducible; no zero-fill, no atomics). */
#define ARFLOW_DENSE_MAX_SRC 8
typedef struct {
  const float* ptr;
  long bstride;
  const float* scale;
} arflow_dense_src;
int arflow_dense_cat_fwd(const float* y, const float* bias, const float* x, float* out, int B, int oc, int C, long HW,
                         float negative_slope, arflow_stream_t stream);
int arflow_dense_gbias_rows(int B, long HW);
int arflow_dense_grad_gather(const arflow_dense_src* srcs, int n_src, const float* act, long act_bs, float* gy,
                             float* gbias_rows, int B, int oc, long HW, float negative_slope, arflow_stream_t stream);

/* ---- bilinear warp ----------------------------------------------------------------------------
 * out[b,c,y,x] = bilinear(src[b,c], x + flow[b,0,y,x], y + flow[b,1,y,x]) with torch grid_sample
 * semantics (pad zeros|border, align_corners) after the reference's normalise/un-normalise round
 * trip.  Replaces flow_warp (utils/warp_utils.py:83-90) and resample(flow_to_warp(.))
 * (utils/uflow_utils.py:6-32,53-77).  src: [B,C,Hs,Ws]; flow: [B,2,H,W] with batch stride
 * flow_bstride floats (>= 2*H*W; lets a [B,4,H,W] tensor be addressed as two flows without a copy);
 * out: [B,C,H,W]; valid (nullable): [B,1,H,W] = mask_invalid(flow_to_warp(flow))
 * (utils/uflow_utils.py:35-50). */
int arflow_warp_fwd(const float* src, const float* flow, float* out, float* valid, int B, int C,
                    int Hs, int Ws, int H, int W, long flow_bstride, int pad_mode, int align_corners,
                    int norm_mode, arflow_stream_t stream);

/* gsrc (nullable, zero-filled here, 4-tap atomic scatter) and gflow (nullable, [B,2,H,W]
 * contiguous).  Deterministic mode: gsrc through the fixed-order scatter of csrc/det_scatter.hip (every element
 * written, no atomics), gflow without the channel split (plain stores). */
int arflow_warp_bwd(const float* gout, const float* src, const float* flow, float* gsrc, float* gflow,
                    int B, int C, int Hs, int Ws, int H, int W, long flow_bstride, int pad_mode,
                    int align_corners, int norm_mode, arflow_stream_t stream);

/* ---- forward-splat maps -----------------------------------------------------------------------
 * variant 0: compute_range_map (utils/uflow_utils.py:80-160, utils/warp_utils.py:158-239)
 * variant 1: get_corresponding_map(grid+flow) (utils/warp_utils.py:26-80) -- clamped indices,
 *            weight zeroed when a tap left the image.
 * out [B,1,H,W] is zero-filled here.  Deterministic mode: the fixed-order scatter of csrc/det_scatter.hip (fp32 sums in
 * ascending source-pixel order instead of 2^-22 fixed point + float atomics; every cell written). */
int arflow_splat_map(const float* flow, float* out, int B, int H, int W, long flow_bstride,
                     int variant, arflow_stream_t stream);

/* mode 0: mask_invalid(flow_to_warp(flow)) closed interval (utils/uflow_utils.py:35-50)
 * mode 1: border_mask(flow) open interval (utils/warp_utils.py:119-134) */
int arflow_coord_mask(const float* flow, float* out, int B, int H, int W, long flow_bstride, int mode,
                      arflow_stream_t stream);

/* get_occu_mask_bidirection (utils/warp_utils.py:93-100): 1 where
 * |f12 + warp(f21,f12)|^2 > scale*(|f12|^2+|warp(f21,f12)|^2) + bias. */
int arflow_occ_bidir(const float* flow12, const float* flow21, float* out, int B, int H, int W,
                     long bstride12, long bstride21, float scale, float bias, arflow_stream_t stream);

/* ---- census / ternary ---------------------------------------------------------------------------
 * Soft census distance between image_a and image_b (both [B,3,H,W], values in [0,1]):
 * ham[b,0,y,x] = sum_k sq/(0.1+sq), sq = (t_a,k - t_b,k)^2, t = d/sqrt(0.81+d^2),
 * d = 255*(gray(y+dy,x+dx) - gray(y,x)) over the (2r+1)^2 patch, zero padding
 * (census_transform + soft_hamming, utils/uflow_utils.py:241-279; TernaryLoss,
 * losses/loss_blocks.py:12-62).
 * If mask != NULL the census_loss reduction (utils/uflow_utils.py:282-293) is fused:
 *   sums[0] += sum (|ham|+0.01)^0.4 * pm,  sums[1] += sum pm,  pm = mask with an r-pixel zero border,
 *   and dham[b,0,y,x] = pm * 0.4*(ham+0.01)^-0.6  (d loss-numerator / d ham) is written instead of ham
 *   when dham != NULL.  sums (2 floats) is zero-filled here.  ham / dham may be NULL. */
int arflow_census_fwd(const float* im_a, const float* im_b, const float* mask, float* ham, float* dham,
                      float* sums, int B, int H, int W, int radius, arflow_stream_t stream);

/* g_im_b[b,c,y,x] = scale[0] * d/d im_b ( sum_p gham[p] * ham[p] ); gham: [B,1,H,W];
 * scale: device scalar (nullable = 1).  Gradient flows into image_b only (call with the images
 * swapped for image_a: the distance is symmetric). */
int arflow_census_bwd(const float* im_a, const float* im_b, const float* gham, const float* scale,
                      float* g_im_b, int B, int H, int W, int radius, arflow_stream_t stream);

/* ---- fused photometric direction of UFlowLoss --------------------------------------------------------
 * losses/uflow_loss.py:30-54 in one launch each way:
 *     recons = resample(im_b, flow_to_warp(flow))                        (utils/uflow_utils.py:6-32,53-77)
 *     mask   = upsample(clamp(occ_small,0,1), x4) * mask_invalid(flow_to_warp(flow))
 *                                               (losses/uflow_loss.py:41-48, utils/uflow_utils.py:35-50,163-182)
 *     sums   = census_loss numerator / denominator of (im_a, recons, mask)   (utils/uflow_utils.py:282-293)
 * The census transform sees only rgb_to_grayscale(image) * 255 (utils/uflow_utils.py:227-231,248), and that is
 * linear like the bilinear sample, so the kernels take the GREY planes gray_a, gray_b [B,1,H,W] (x255, from
 * arflow_down4_gray) and sample one plane instead of three; the warped image, its gradient and the validity mask
 * never exist in memory.  Equal to arflow_warp_fwd + arflow_up4_clamp_mul + arflow_census_fwd up to fp32
 * re-association.
 * flow: [B,2,H,W] with batch stride flow_bstride; occ_small: [B,1,H/4,W/4] (the range map of arflow_splat_map;
 * NULL = no occlusion term, mask = validity only); mask_out: [B,1,H,W] or NULL; dham: [B,1,H,W] (saved for the
 * backward); sums: as arflow_census_fwd (zero-filled here).
 * Needs H % 4 == 0 and W % 4 == 0 (arflow_census_warp_supported() == 1), else ARFLOW_ESHAPE. */
int arflow_census_warp_supported(int H, int W);
int arflow_census_warp_fwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                           const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H, int W,
                           int radius, arflow_stream_t stream);
/* gflow[B,2,H,W] = scale[0] * d(sums[0]) / d flow through the census distance and the bilinear sample
 * (= arflow_census_bwd followed by arflow_warp_bwd with gsrc = NULL).  scale: device scalar or NULL (= 1). */
int arflow_census_warp_bwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                           const float* dham, const float* scale, float* gflow, int B, int H, int W, int radius,
                           arflow_stream_t stream);
/* Both directions of UFlowLoss (losses/uflow_loss.py:30-54 runs them one after the other) in ONE launch each way: the batch
 * holds B2 = 2 x image pairs, sample s = 2 b + direction -- the model's [B,4,H,W] (fw, bw) flow tensor viewed as [2B,2,H,W]
 * and the [B,6,H,W] image pair viewed as [2B,3,H,W].  `gray`: the 2B grey planes (arflow_down4_gray on that view): image a
 * of sample s is plane s, image b plane s ^ 1; occ_small plane s ^ 1 (range map of the partner direction's level-2 flow)
 * masks sample s.  sums: columns (0, 1) = (sum loss, sum mask) of direction 0, (2, 3) of direction 1.  scale2: two
 * factors, one per direction. */
int arflow_census_warp_pair_fwd(const float* gray, const float* flow, long flow_bstride, const float* occ_small,
                                float* mask_out, float* dham, float* sums, int B2, int H, int W, int radius,
                                arflow_stream_t stream);
int arflow_census_warp_pair_bwd(const float* gray, const float* flow, long flow_bstride, const float* dham,
                                const float* scale2, float* gflow, int B2, int H, int W, int radius, arflow_stream_t stream);
/* The whole backward of UFlowLoss as ONE launch: arflow_census_warp_pair_bwd (-> gflow [B2,2,H,W]) and arflow_smooth_bwd of
 * the level-2 flows flow2 [B2,2,h2,w2] with the x1/4 images img2 [B2,3,h2,w2] and the two sum gradients coef2
 * (-> gflow2 [B2,2,h2,w2]) as workgroup roles of one kernel. */
int arflow_uflow_pair_bwd(const float* gray, const float* flow, long flow_bstride, const float* dham, const float* scale2,
                          float* gflow, int B2, int H, int W, int radius, const float* flow2, long flow2_bstride,
                          const float* img2, const float* coef2, float* gflow2, int h2, int w2, float flow_scale, float alpha,
                          int order, int wmode, int penalty, arflow_stream_t stream);
/* gray[B,1,H,W] = rgb_to_grayscale(im) * 255 (utils/uflow_utils.py:227-231) and, if small != NULL,
 * small[B,3,H/4,W/4] = downsample(im, x1/4) as arflow_down4 (losses/uflow_loss.py:59-60) from the same read.
 * im: [B,3,H,W], H % 4 == 0, W % 4 == 0. */
int arflow_down4_gray(const float* im, float* small, float* gray, int B, int H, int W, arflow_stream_t stream);
/* As arflow_down4_gray; additionally clears zero_plane ([B, H/4, W/4] floats, nullable): the accumulation target of the
 * range-map splat that follows (arflow_splat_smooth_fwd with prezeroed = 1), saving its fill launch. */
int arflow_down4_gray_z(const float* im, float* small, float* gray, float* zero_plane, int B, int H, int W,
                        arflow_stream_t stream);
/* compute_range_map(flow) (utils/uflow_utils.py:80-160; arflow_splat_map variant 0) AND the edge-aware smoothness sums of
 * arflow_smooth_fwd(flow, img [B,3,H,W], ...) (losses/uflow_loss.py:62-102) in ONE launch: UFlowLoss needs both of the same
 * level-2 flows.  out: [B,1,H,W] range map (prezeroed != 0: the caller guarantees it arrives zero-filled); sums as for
 * arflow_smooth_fwd.  The smoothness backward is arflow_smooth_bwd. */
int arflow_splat_smooth_fwd(const float* flow, const float* img, float* out, float* sums, int B, int H, int W,
                            long flow_bstride, float flow_scale, float alpha, int order, int wmode, int penalty, int prezeroed,
                            arflow_stream_t stream);


/* ---- SSIM + L1 photometric term (losses/flow_loss.py:13-27, losses/loss_blocks.py:65-84) --------
 * x = recons*mask, y = im*mask, 3x3 un-padded box SSIM, dist = clamp((1-SSIM)/2,0,1).
 * sums[0] += sum |im-recons|*mask  (B*C*H*W terms)
 * sums[1] += sum dist              (B*C*(H-2)*(W-2) terms)
 * sums[2] += sum mask              (B*H*W terms)
 * ssim_map (nullable): [B,C,H-2,W-2].  mask nullable (= ones).  sums: slotted, 3 quantities. */
int arflow_photo_fwd(const float* im, const float* recons, const float* mask, float* ssim_map,
                     float* sums, int B, int C, int H, int W, arflow_stream_t stream);

/* g_recons = coef[0] * d sums[0]/d recons + coef[1] * d sums[1]/d recons, or, when gmap != NULL,
 * coef[0] * dL1 + sum_w gmap[w] * d dist[w] / d recons.  coef: 2 device floats. */
int arflow_photo_bwd(const float* im, const float* recons, const float* mask, const float* gmap,
                     const float* coef, float* g_recons, int B, int C, int H, int W,
                     arflow_stream_t stream);

/* ---- fused warp + mask + L1/SSIM pass of one pyramid scale (unFlowLoss, MvLoss) ---------------------
 * N = G * B samples in G groups (directions / views) of B.  For sample (g, b):
 *   rec = flow_warp(src, flow, pad_mode)            bilinear, align_corners=True (utils/warp_utils.py:83-90)
 *   rows -> per group  sum |tgt - rec| * m,  sum SSIMdist(rec * m, tgt * m),  sum m   (the sums of arflow_photo_fwd)
 * Nothing is copied to feed it: target image, source image ([C,H,W] planes, 1 <= C <= 3, else ARFLOW_EPARAM), flow
 * ([2,H,W]) and mask plane of sample (g, b) start at  base + b * X_bs + g * X_half  floats (X_half may be negative), so
 * two images inside one [B,6,H,W] tensor, a [B,4,H,W] flow pair or two separate tensors are read in place.
 * mask_mode: ARFLOW_PW_MASK_PLANE    m = mask[y, x] of an [H,W] plane;
 *            ARFLOW_PW_MASK_NEAREST  m = mask[y * (mask_h / H), x * (mask_w / W)] of a [mask_h, mask_w] plane -- the
 *                                    F.interpolate(mode='nearest') resize for integer factors (others: ARFLOW_ESHAPE);
 *            ARFLOW_PW_MASK_BORDER   m = border_mask(flow) (utils/warp_utils.py:119-134; `mask` is ignored).
 * mask_invert != 0 uses 1 - m instead.  mask_out (nullable): [N,1,H,W], receives the plane actually used.
 * rows: arflow_photo_warp_rows(N, H, W) rows of ARFLOW_SUM_COLS floats, one per 16 x 64 tile in (sample, tile row,
 * tile column) order, every one written by the call: group g owns rows [g, g + 1) * rows / G and quantity k of the
 * group is the sum of column k over them.  No atomics: bitwise reproducible.  H, W >= 3. */
#define ARFLOW_PW_MASK_PLANE 0
#define ARFLOW_PW_MASK_NEAREST 1
#define ARFLOW_PW_MASK_BORDER 2
int arflow_photo_warp_rows(int N, int H, int W);
int arflow_photo_warp_fwd(const float* tgt, long tgt_bs, long tgt_half, const float* src, long src_bs, long src_half,
                          const float* flow, long flow_bs, long flow_half, const float* mask, long mask_bs,
                          long mask_half, int mask_mode, int mask_invert, int mask_h, int mask_w, float* mask_out,
                          float* rows, int B, int G, int C, int H, int W, int pad_mode, arflow_stream_t stream);

/* d/d flow of  sum_g coef[2g] * (L1 sum of group g) + coef[2g+1] * (SSIM sum of group g)  (coef: 2 G device floats; the
 * mask sum has no gradient), written for sample (g, b) at  gflow + b * gflow_bs + g * gflow_half  ([2,H,W]): the
 * gradient of the tensor the flow was read from, so no slice / cat backward is needed.  Warp, mask and window statistics
 * are recomputed; every pixel owns its two outputs (pure gather, no atomics).  No gradient w.r.t. the images. */
int arflow_photo_warp_bwd(const float* tgt, long tgt_bs, long tgt_half, const float* src, long src_bs, long src_half,
                          const float* flow, long flow_bs, long flow_half, const float* mask, long mask_bs,
                          long mask_half, int mask_mode, int mask_invert, int mask_h, int mask_w, const float* coef,
                          float* gflow, long gflow_bs, long gflow_half, int B, int G, int C, int H, int W, int pad_mode,
                          arflow_stream_t stream);

/* Every F.interpolate(frames, (h, w), mode='area') copy of a pyramid loss in one launch.  frames: [planes,H,W];
 * sizes: HOST array of n (h, w) pairs, n <= ARFLOW_AREA_PYRAMID_MAX (else ARFLOW_EPARAM), h | H and w | W (else
 * ARFLOW_ESHAPE).  Pair i with a factor > 1 is written as [planes,h,w] behind the pairs before it in the packed `out`
 * (arflow_area_pyramid_ws_bytes() bytes in all); a pair with h == H and w == W produces nothing.  Every scale is
 * computed from the full-resolution pixels; a block's pixels are added as lane partials that meet in a shuffle tree. */
#define ARFLOW_AREA_PYRAMID_MAX 8
long arflow_area_pyramid_ws_bytes(int planes, int H, int W, const int* sizes, int n);
int arflow_area_pyramid(const float* frames, float* out, int planes, int H, int W, const int* sizes, int n,
                        arflow_stream_t stream);

/* ---- edge-aware smoothness ------------------------------------------------------------------------
 * sums[0] += sum_{b,ch,y,x} wx * pen(Dx flow),  sums[1] += sum wy * pen(Dy flow)
 * order 1: Dx f = f[x+1]-f[x];           wx = exp(-alpha * mean_c |img[x+1]-img[x]|)
 * order 2: Dx f = f[x+2]-2f[x+1]+f[x];   wx from img[x+2]-img[x+1] (wmode 0, smooth_grad_2nd,
 *          losses/loss_blocks.py:112-124) or img[x+2]-img[x] (wmode 1, UFlowLoss smooth_order 2,
 *          losses/uflow_loss.py:81-102)
 * penalty 0: |v| (loss_blocks.py:101-103), 1: sqrt(v^2 + 1e-6) (penalty_uflow :8-9, robust_l1(v^2)
 * utils/uflow_utils.py:337-338).  flow: [B,2,H,W] (batch stride flow_bstride), flow values are
 * multiplied by flow_scale first; img: [B,Ci,H,W].  sums: slotted, 2 quantities. */
int arflow_smooth_fwd(const float* flow, const float* img, float* sums, int B, int Ci, int H, int W,
                      long flow_bstride, float flow_scale, float alpha, int order, int wmode, int penalty,
                      arflow_stream_t stream);

/* gflow ([B,2,H,W] contiguous) = coef[0]*d sums[0]/d flow + coef[1]*d sums[1]/d flow. */
int arflow_smooth_bwd(const float* flow, const float* img, const float* coef, float* gflow, int B, int Ci,
                      int H, int W, long flow_bstride, float flow_scale, float alpha, int order, int wmode,
                      int penalty, arflow_stream_t stream);

/* ---- resize helpers ---------------------------------------------------------------------------------
 * downsample(img, x1/4) of utils/uflow_utils.py:185-204 for H,W multiples of 4 (= mean of the central
 * 2x2 of each 4x4 block); in [B*C,H,W] -> out [B*C,H/4,W/4]. */
int arflow_down4(const float* in, float* out, int planes, int H, int W, arflow_stream_t stream);

/* out[b,0,y,x] = bilinear x4 upsample (align_corners=False, utils/uflow_utils.py:163-182) of
 * clamp(in,0,1) times valid (nullable): the occlusion-mask assembly of losses/uflow_loss.py:41-48.
 * in [B,1,h,w]; valid/out [B,1,4h,4w]. */
int arflow_up4_clamp_mul(const float* in, const float* valid, float* out, int B, int h, int w,
                         arflow_stream_t stream);

/* ---- ground-truth flow metrics -----------------------------------------------------------------------
 * The sums behind evaluate_flow (utils/flow_utils.py:121-183; trainer/uflow_trainer.py:94-170 validates with it after every
 * epoch) in ONE launch, without bringing the flow to the host.  Per ground-truth pixel, fp32, in the reference's order:
 *   u = (pred_u / w) * W, v = (pred_v / h) * H                                             (flow_utils.py:139-140)
 *   bilinear resize to H x W, half-pixel rule (cv2.resize INTER_LINEAR, :143 = ATen upsample_bilinear2d(align_corners=False))
 *   epe = sqrt(du^2 + dv^2) against gt[:, 0:2]                                             (:145-146)
 *   valid = gt[:, 2], noc = gt[:, 3] (C = 4, read as [..., 2] and [..., -1], :151-152; both 1 for C = 2)
 *   bad = (e > 3) && (e / max(|gt|, 1e-10) > 0.05), e = epe * valid                        (:123-128)
 * rows: [B][arflow_flow_eval_rows(H, W)][8] doubles, need not be initialised: every row is stored by the call (one row per
 * workgroup -- the `sums` conventions above; no zero-fill launch, no atomics: bitwise reproducible in either mode).  A
 * sample's quantity k is the sum of column k over its rows:
 *   0 sum epe*valid   1 sum valid   2 sum epe*noc   3 sum noc   4 sum bad   5 sum epe*valid*move   6 sum valid*move   7 zero
 * (move NULL: columns 5, 6 are 0).  The occluded and the static sums follow on the host: (0) - (2), (1) - (3) and
 * (0) - (5), (1) - (6).  Partials are fp32 per thread over 8 pixels and double from the wave reduction on.
 * pred: [B,2,h,w]; gt: [B,C,H,W], C = 2 or 4 (else ARFLOW_EPARAM); move: [B,1,H,W] or NULL (needs C = 4, else
 * ARFLOW_EPARAM); epe_map: [B,1,H,W] or NULL.  Any h, w, H, W >= 1 (float4 rows when W % 4 == 0 and gt / move / epe_map
 * are 16-byte aligned).  arflow_flow_eval_rows: rows per sample, or ARFLOW_ESHAPE. */
int arflow_flow_eval_rows(int H, int W);
int arflow_flow_eval(const float* pred, const float* gt, const float* move, double* rows, float* epe_map, int B, int h,
                     int w, int C, int H, int W, arflow_stream_t stream);

/* ---- sparse triangular solves on the pixel grid -----------------------------------------------------------
 * forward_substitution / backward_substitution / inverse_diagonal of utils/triag_solve.py:76-115 and utils/triag_solve/
 * triag_solve_cuda.cu:72-139: the sparse Cholesky factor of the precision of losses/uflow_elbo_loss.py:149-157, a pixel
 * coupled to three neighbours.  P = K * L planes, fp32, contiguous: A [P,M,N], B [P,M,N-1], C [P,M-1,N], D [P,M-1,N-1].
 *   lower (upper = 0): A[i,j] y[i,j] + B[i,j-1] y[i,j-1] + C[i-1,j] y[i-1,j] + D[i-1,j-1] y[i-1,j-1] = x[i,j]   (:84-92)
 *   upper (upper = 1): A[i,j] y[i,j] + B[i,j] y[i,j+1] + C[i,j] y[i+1,j] + D[i,j] y[i+1,j+1] = x[i,j]           (:105-113)
 * One wave per plane, one lane per row, rows skewed by one column each so that the wave walks the anti-diagonals; rows
 * beyond 64 in further strips of the same wave: ceil(M / 64) * (N + 63) dependent steps, not M * N.
 * Per element the rounded C, B and D products are subtracted in the reference's order and the result is divided by A
 * (IEEE): the bits of the reference's fp32 CPU run, on every run and in either mode (no atomics).
 * arflow_triag_solve: Y = J^-1 X.  D may be NULL (zero); B, C, D may be NULL where they have no elements (N == 1, M == 1).
 * arflow_triag_solve_bwd: the whole backward of ForwardSubst (upper = 0) / BackwardSubst (upper = 1) of :163-202 in one
 *   launch.  Y: the forward's result.  gX = the solve of the transposed system (the opposite triangle, the same arrays) on
 *   gY; gA = -gX * Y, and gB, gC, gD the products of :178-180 / :199-201, stored as the sweep produces gX: every element
 *   of all five is stored.  gD is NULL exactly when D is (ARFLOW_ENULL / ARFLOW_EPARAM otherwise); gB, gC as B, C.
 * arflow_triag_inverse_diagonal: H[p,k,l] = |J^-1 e_(k,l)|^2 for the lower form without D = the diagonal of (J J^T)^-1
 *   (marginal_variances, :205-218).  One wave per source pixel on the rows >= k and columns >= l its solution can reach;
 *   the squares are summed in registers -- no scratch tensor.
 * Limits (ARFLOW_ESHAPE beyond them): M <= 16384, N <= 8192 (a strip's last row is kept in LDS), and for
 * arflow_triag_inverse_diagonal P * M * N < 2^31.  X and Y (gY and gX) must not overlap. */
int arflow_triag_solve(const float* A, const float* B, const float* C, const float* D, const float* X, float* Y, int P,
                       int M, int N, int upper, arflow_stream_t stream);
int arflow_triag_solve_bwd(const float* A, const float* B, const float* C, const float* D, const float* Y, const float* gY,
                           float* gX, float* gA, float* gB, float* gC, float* gD, int P, int M, int N, int upper,
                           arflow_stream_t stream);
int arflow_triag_inverse_diagonal(const float* A, const float* B, const float* C, float* H, int P, int M, int N,
                                  arflow_stream_t stream);

/* ---- the banded operator of the sparse-covariance family and its fused sampler (csrc/band.hip) ---------------
 * matrix_vector_product_general / matrix_vector_product_T_general of utils/triag_solve.py:29-43, :59-73 and the sampler
 * z = mean + L eps of losses/uflow_elbo_loss.py:142-147.  0 <= k <= 3; tap (i, j), 0 <= i, j <= k, has
 * index ind = i (k + 1) + j; its coefficient plane for channel c in {0, 1} is channel c of `diag` (ind = 0) or channel
 * 2 (ind - 1) + c of `off` (ind >= 1; `off` may be NULL when k = 0).  Sample s of batch item b is plane s B + b of X, Y, gY
 * and gX.  Every tensor is fp32 with contiguous [2 or 2 ((k+1)^2 - 1)][M][N] items and its OWN batch stride in floats (read
 * only when there is a second item), so channel slices of wider tensors are passed in place.
 *   transpose = 0:  Y[sB+b,c,y,x] = mean[b,c,y,x] + sum_ind A[b,ind,c,y-i,x-j] X[sB+b,c,y-i,x-j]    (terms on the grid)
 *   transpose = 1:  Y[sB+b,c,y,x] = mean[b,c,y,x] + sum_ind A[b,ind,c,y,x] X[sB+b,c,y+i,x+j]
 * mean may be NULL (no addition).  Per element the products are rounded and added in ind order starting from 0, then added
 * to the mean: the bits of the reference's fp32 CPU run.  The coefficients of a batch item are read once per launch for all
 * S samples.
 * arflow_band_mv_bwd, one launch, for the forward of orientation `transpose` with G = gY:
 *   gX = the product of the OTHER orientation of G (NULL: not wanted);  gmean[b] = sum_s G[sB+b] (NULL: not wanted);
 *   gA[b,ind,c,y,x] = sum_s X[sB+b,c,y,x] G[sB+b,c,y+i,x+j] (transpose = 0) or sum_s G[sB+b,c,y,x] X[sB+b,c,y+i,x+j]
 *   (transpose = 1), stored to gdiag / goff in the layout of diag / off.  Every element of every output is stored; sums run
 *   in a fixed order in one thread (no atomics: the same bits in either mode).
 * ARFLOW_ENULL: a required pointer is NULL (off / goff only when k > 0); ARFLOW_EPARAM: k outside 0..3 or transpose not 0 / 1;
 * ARFLOW_ESHAPE: B, S, M or N < 1, a batch stride smaller than its item, M N >= 2^31, B > 32767 or M > 524280.  Outputs
 * must not overlap inputs. */
int arflow_band_mv_fwd(const float* mean, long mean_bs, const float* diag, long diag_bs, const float* off, long off_bs,
                       const float* X, long x_bs, float* Y, long y_bs, int B, int S, int M, int N, int k, int transpose,
                       arflow_stream_t stream);
int arflow_band_mv_bwd(const float* diag, long diag_bs, const float* off, long off_bs, const float* X, long x_bs,
                       const float* gY, long gy_bs, float* gX, long gx_bs, float* gmean, long gmean_bs, float* gdiag,
                       long gdiag_bs, float* goff, long goff_bs, int B, int S, int M, int N, int k, int transpose,
                       arflow_stream_t stream);

/* ---- the low-rank covariance family: fused sampler, Gram log-determinant, one backward (csrc/lowrank.hip) ------
 * reparam_lowrank and the entropy of approx 'lowrank' of losses/uflow_elbo_loss.py:180-188, :362-381.
 * std [B][2R][M][N]: channel 2k + c is column k of flow component c in {0, 1}; 1 <= R <= 16; p = y N + x.  Sample s of batch
 * item b is plane s B + b of Z, gZ and row s B + b of eps [S B][2R] (contiguous).  Every tensor is fp32 with contiguous planes
 * and its OWN batch stride in floats (read only when there is a second item), so channel slices are passed in place.
 *   arflow_lowrank_sample_fwd:  Z[sB+b,c,p] = mean[b,c,p] + sum_k std[b,2k+c,p] eps[sB+b,2k+c]; the products are rounded and
 *     added in k order onto the mean.  std is read once for all S samples.
 *   arflow_lowrank_logdet_fwd:  G[b,c] = U U^T with U = std[b, c::2] as [R][M N], accumulated in float64 (exact products);
 *     logdet [B][2] = log det G and ginv [B][2][R][R] = G^-1, from a float64 Cholesky factorisation, rounded once to fp32.
 *     work: arflow_lowrank_work_size(B, R, M, N) doubles (< 0: the ARFLOW_E* code), need not be initialised.  Two launches;
 *     a pivot that is not positive gives NaN for that (b, c)'s logdet and ginv (no host synchronisation).
 *   arflow_lowrank_bwd, one launch:  gmean[b,c,p] = sum_s gZ[sB+b,c,p] (NULL: not wanted);
 *     gstd[b,2i+c,p] = sum_s eps[sB+b,2i+c] gZ[sB+b,c,p] + 2 glogdet[b,c] sum_j ginv[b,c,i,j] std[b,2j+c,p].  gZ may be NULL
 *     (no sampler term; eps is then not read) and glogdet [B][2] (a DEVICE pointer) may be NULL (no log-det term; ginv is
 *     then not read).
 * No atomics: the same bits in either mode.  Every element of every output is stored.
 * ARFLOW_ENULL: a required pointer is NULL; ARFLOW_EPARAM: R outside 1..16; ARFLOW_ESHAPE: B, S, M or N < 1, a batch stride
 * smaller than its item, M N >= 2^31, B > 32767.  Outputs must not overlap inputs. */
int arflow_lowrank_sample_fwd(const float* mean, long mean_bs, const float* std, long std_bs, const float* eps, float* Z,
                              long z_bs, int B, int S, int R, int M, int N, arflow_stream_t stream);
long arflow_lowrank_work_size(int B, int R, int M, int N);
int arflow_lowrank_logdet_fwd(const float* std, long std_bs, double* work, float* logdet, float* ginv, int B, int R, int M,
                              int N, arflow_stream_t stream);
int arflow_lowrank_bwd(const float* std, long std_bs, const float* eps, const float* gZ, long gz_bs, const float* ginv,
                       const float* glogdet, float* gmean, long gmean_bs, float* gstd, long gstd_bs, int B, int S, int R,
                       int M, int N, arflow_stream_t stream);

/* ---- the Gaussian-mixture family: fused sampler + mixture log-density, one backward, entropy map (csrc/mixture.hip) ------
 * reparam_gmm and the entropy of approx 'mixture' of losses/uflow_elbo_loss.py:159-178, :358-361 with gaussian_mixture_log_pdf
 * and mixture_entropy of utils/misc_utils.py:67-132.
 * mean, log_std [B][2K][M][N]: channel 2k + c is flow component c of mixture component k; 1 <= K <= 4; p = y N + x, P = M N.
 * weights [B][K] >= 0 (contiguous); comp [B][S] 64-bit integers (contiguous): the component sample s of item b is drawn from,
 * a value outside 0..K-1 is clamped into it; eps [S B][2][M][N].  Sample s of item b is row n = s B + b of eps, flow, gZ and
 * of logpdf [S B], resp [S B][K], q [S B][K] (contiguous).  Every image-like tensor is fp32 with contiguous planes and its
 * OWN batch stride in floats (read only when there is a second item), so channel slices are passed in place.
 *   arflow_mixture_sample_fwd, one launch:  z = comp[b][s];  flow[n,c,p] = mean[b,2z+c,p] + exp(log_std[b,2z+c,p]) eps[n,c,p]
 *     in fp32 (the product rounded, then the sum), and float64 partial sums over CHUNK = 1024 consecutive pixels of
 *       A[n,k] = -sum_p sum_c (log_std[b,2k+c,p] + d^2 / 2),  d = (flow[n,c,p] - mean[b,2k+c,p]) / exp(log_std[b,2k+c,p])
 *     into work [S B][chunks][K]: arflow_mixture_work_size(B, S, K, M, N) doubles (< 0: the ARFLOW_E* code), need not be
 *     initialised.  float4 groups when P % 4 == 0 and all planes are 16-byte aligned, scalar loads otherwise.
 *   arflow_mixture_logpdf_fwd, one small launch: adds the partials in chunk order and writes, from float64 rounded once,
 *       logpdf[n] = (max_k A + log sum_k w[b,k] exp(A[n,k] - max_k A)) / P
 *       resp[n,k] = w[b,k] e_k / sum_j w[b,j] e_j,   q[n,k] = e_k / sum_j w[b,j] e_j,   e_k = exp(A[n,k] - max_k A)
 *     (w[b,k] = 0 gives resp = 0 and a finite q).  d logpdf[n] / d w[b,k] = q[n,k] / P.
 *   arflow_mixture_bwd, one launch, a gather (one thread per pixel of item b loops over s and k); with lambda[n] =
 *     glogpdf[n] / P and G[n,c,p] = gZ[n,c,p] - lambda[n] sum_k resp[n,k] d / std:
 *       gmean[b,2k+c,p]    = sum_s (lambda[n] resp[n,k] d / std + [z == k] G[n,c,p])
 *       glog_std[b,2k+c,p] = sum_s (lambda[n] resp[n,k] (d^2 - 1) + [z == k] G[n,c,p] std[b,2k+c,p] eps[n,c,p])
 *     The samples are recomputed from eps (the sampler's own fp32 expression).  glogpdf [S B] (a DEVICE pointer) may be NULL
 *     (no density term; resp is then not read) and gZ may be NULL (no gradient into the samples).
 *   arflow_mixture_entropy_map, one launch, forward only:  out[b,p] = -(1 / n) sum_i (max_k x_k + log sum_k w[b,k] exp(x_k -
 *     max)), x_k = -sum_c (log_std + d^2 / 2) at the pixel, for the n draws comp [B][n], eps [n B][2][M][N] (draw i of item b is
 *     row i B + b); out [B][M N] contiguous.  mean and log_std are read once per pixel.
 * No atomics: the same bits in either mode.  Every element of every output is stored.
 * ARFLOW_ENULL: a required pointer is NULL; ARFLOW_EPARAM: K outside 1..4; ARFLOW_ESHAPE: B, S (n), M or N < 1, a batch
 * stride smaller than its item, M N >= 2^31, S B > 65535.  Outputs must not overlap inputs. */
long arflow_mixture_work_size(int B, int S, int K, int M, int N);
int arflow_mixture_sample_fwd(const float* mean, long mean_bs, const float* log_std, long ls_bs, const float* eps, long eps_bs,
                              const long* comp, float* flow, long flow_bs, double* work, int B, int S, int K, int M, int N,
                              arflow_stream_t stream);
int arflow_mixture_logpdf_fwd(const double* work, const float* weights, float* logpdf, float* resp, float* q, int B, int S,
                              int K, int M, int N, arflow_stream_t stream);
int arflow_mixture_bwd(const float* mean, long mean_bs, const float* log_std, long ls_bs, const float* eps, long eps_bs,
                       const long* comp, const float* resp, const float* glogpdf, const float* gZ, long gz_bs, float* gmean,
                       long gmean_bs, float* glog_std, long gls_bs, int B, int S, int K, int M, int N, arflow_stream_t stream);
int arflow_mixture_entropy_map(const float* mean, long mean_bs, const float* log_std, long ls_bs, const float* weights,
                               const long* comp, const float* eps, long eps_bs, float* out, int B, int n, int K, int M, int N,
                               arflow_stream_t stream);

/* ---- the diagonal Gaussian sampler of ElboLoss over a whole pyramid ------------------------
 * losses/elbo_loss.py:17-27,90-91,117-124 for all n scales (1 <= n <= 6, else ARFLOW_EPARAM) in ONE launch.  Every argument
 * that is an array has n entries on the HOST (pointers to device tensors, batch strides in floats, sizes); the tables travel
 * to the kernel by value.  Per scale i:
 *   net[i] [B][8][h_i][w_i]: mean_fw 0:2, logvar_fw 2:4, mean_bw 4:6, logvar_bw 6:8;  eps[i], z[i] [B][4][h_i][w_i]: the
 *   forward direction in channels 0:2, the backward one in 2:4.  fp32, planes contiguous, each tensor with its own batch
 *   stride (read only when B > 1): channel slices are passed in place.
 * arflow_gauss_pyr_sample_fwd:  z = mean + RN(expf(logvar / 2) * eps) in fp32, and ent [n][2] (float64, device):
 *   ent[i][d] = sum over b, the two channels and the pixels of logvar_d, in float64 from the load on -- per lane, by wave
 *   butterfly, in wave order: one partial per workgroup in work (arflow_gauss_pyr_work_size(h, w, n, B) doubles, < 0: the
 *   ARFLOW_E* code; need not be initialised), folded in a fixed order by a second one-wave-per-sum launch of the same call.
 * arflow_gauss_pyr_sample_bwd, one launch, a per-pixel map that stores all 8 channels of every gnet[i] [B][8][h_i][w_i]:
 *   gmean = gz,  glogvar = gz * (0.5f * expf(logvar / 2) * eps) + (float)gent[i][d]
 *   gz (the array, or an entry of it) may be NULL: zero.  gent [n][2] is a DEVICE pointer (float64) or NULL (zero).  The
 *   standard deviation is recomputed with the sampler's expression.
 * float4 groups for a scale whose h w % 4 == 0 with 16-byte aligned pointers and strides, scalar accesses otherwise.  No
 * atomics: the same bits in either mode.  Every element of every output is stored.
 * ARFLOW_ENULL: a required pointer (or entry) is NULL; ARFLOW_EPARAM: n outside 1..6; ARFLOW_ESHAPE: B, h or w < 1, B > 65535,
 * h w >= 2^30, a batch stride smaller than its item, more than 2^31 - 1 workgroups.  Outputs must not overlap inputs. */
long arflow_gauss_pyr_work_size(const int* h, const int* w, int n, int B);
int arflow_gauss_pyr_sample_fwd(const float* const* net, const long* net_bs, const float* const* eps, const long* eps_bs,
                                float* const* z, const long* z_bs, const int* h, const int* w, int n, int B, double* work,
                                double* ent, arflow_stream_t stream);
int arflow_gauss_pyr_sample_bwd(const float* const* gz, const long* gz_bs, const float* const* net, const long* net_bs,
                                const float* const* eps, const long* eps_bs, const double* gent, float* const* gnet,
                                const long* gnet_bs, const int* h, const int* w, int n, int B, arflow_stream_t stream);

/* ---- MseLoss: squared error against the resized ground-truth flow --------------------------
 * losses/mse_loss.py:9-148 and resize_flow of utils/flow_utils.py:110-118.  fp32, planes contiguous, each tensor with its
 * own batch stride in floats (read only when it has more than one item): channel slices are passed in place.
 *   net [B][C][h][w]: mean 0:2, log_diag 2:4, and in mode 2 left 4:6 (without its last column) and over 6:8 (without its
 *   last row);  target [B][2][H][W], any H, W >= 1;  ez [S B][2][h][w], sample s of item b at index s B + b.
 *   mode 0: ez is the noise, z = mean + RN(expf(log_diag) ez);  mode 1: z = mean + RN(expf(-log_diag) ez);
 *   mode 2: ez IS z (written by the 4-neighbour samplers).  align_corners 0 / 1: the taps of the bilinear resize.
 * gt = resize_flow(target, (h, w)): the source coordinate in float64, the weights rounded to fp32 once, ATen's fp32 blend,
 * the division by W / w (channel 0) and H / h (channel 1) in float64 rounded once.  r = z - gt in fp32.
 * arflow_mse_fwd: sums [4] (float64, device) = { sum r^2 over all S B 2 h w elements, sum log_diag over B 2 h w, sum left^2,
 *   sum over^2 (both 0 in modes 0 and 1) }, accumulated in float64 from r / the load on: per lane, by wave butterfly, in wave
 *   order, one row of 4 partials per workgroup in work (arflow_mse_work_size(B, h, w) doubles, < 0: the ARFLOW_E* code; need
 *   not be initialised), folded in a fixed order by a second one-wave launch of the same call.  z is never stored.
 * arflow_mse_bwd, one launch; gsums [4] (float64, DEVICE) is the gradient with respect to sums.  With c = (float)(2 gsums[0]),
 *   ge = (float)gsums[1], gz = c r:
 *   modes 0, 1: gnet[:, 0:2] = sum_s gz, gnet[:, 2:4] = sum_s gz (+- RN(std ez)) + ge (minus in mode 1), channels 4.. zero;
 *               gz may be NULL;
 *   mode 2:     gz [S B][2][h][w] = c r (required), gnet[:, 0:2] = 0, [:, 2:4] = ge, [:, 4:6] = (float)(2 gsums[2]) left,
 *               [:, 6:8] = (float)(2 gsums[3]) over (zero in the column / row the slices leave out), channels 8.. zero.
 * arflow_resize_flow: out [B][2][h][w] = gt alone.
 * No atomics: the same bits in either mode.  Every element of every output is stored.
 * ARFLOW_ENULL: a required pointer is NULL;  ARFLOW_EPARAM: mode outside 0..2, align_corners outside 0 / 1, an output that
 * overlaps an input or another output;  ARFLOW_ESHAPE: B, S, h, w, H or W < 1, S B > 65535 (B > 65535 for the resize), a plane
 * of 2^30 or more elements, C < 4 (C < 8, h < 2 or w < 2 in mode 2), a batch stride smaller than its item. */
long arflow_mse_work_size(int B, int h, int w);
int arflow_mse_fwd(const float* net, long net_bs, int C, const float* target, long target_bs, int H, int W, const float* ez,
                   long ez_bs, int B, int S, int h, int w, int mode, int align_corners, double* work, double* sums,
                   arflow_stream_t stream);
int arflow_mse_bwd(const float* net, long net_bs, int C, const float* target, long target_bs, int H, int W, const float* ez,
                   long ez_bs, const double* gsums, float* gnet, long gnet_bs, float* gz, long gz_bs, int B, int S, int h, int w,
                   int mode, int align_corners, arflow_stream_t stream);
int arflow_resize_flow(const float* flow, long flow_bs, int H, int W, float* out, long out_bs, int B, int h, int w,
                       int align_corners, arflow_stream_t stream);

/* ---- uncertainty metrics: sparsification curves and the calibration histogram -----------------------------------
 * The device side of evaluate_uncertainty / sp_plot / CalibrationCurve of utils/flow_utils.py:186-320 (DESIGN.md section
 * 19).  The `rows` conventions of arflow_flow_eval hold for all three: a row buffer need not be initialised, every row is
 * stored by exactly one workgroup, no atomics and no zero-fill launch, bitwise reproducible in either mode.
 * arflow_uncert_prep: ent [B,2,h,w] -> ent_map [B,1,H,W] = sum over the two channels of the bilinear resize (half-pixel
 *   rule, as arflow_flow_eval) of (ent[:,0] - sub_w) + add_W and (ent[:,1] - sub_h) + add_H, every step rounded to fp32 in
 *   that order (:296-307; the caller passes (float)(2 log w), (float)(2 log W), (float)(2 log h), (float)(2 log H)).
 *   rows [B][arflow_uncert_rows(H, W)][8]: min ent_map, max ent_map, min epe_map, max epe_map, sum valid, 0, 0, 0 per tile
 *   -- columns 0..3 fold with min / max, column 4 with a sum.  epe_map [B,1,H,W] (arflow_flow_eval's output); valid: the
 *   validity plane of sample 0, sample b at valid + b * valid_bstride (gt + 2 H W with stride C H W), or NULL (all ones).
 * arflow_sparsify_sums: rows [B][arflow_uncert_rows(H, W)][F][K][3], F = 2 if field1 else 1, 1 <= K <= 32 (else
 *   ARFLOW_EPARAM): per sample, field and threshold thr[b][f][k] (doubles on the device)
 *     0 sum (1 - m) g     1 sum m g     2 sum err m g,      m = 1 / (1 + expf(-a)), a = alpha * d (fp32),
 *   d = (float)(thr - (double)field): the difference is formed in double, expf is the accurately rounded one.  Partials
 *   are fp32 per thread over 8 pixels and double from the wave reduction on.  err, field0, field1: [B,1,H,W].
 * arflow_calib_hist: pred [B,2,H,W], gt [B,C,H,W] (C = 2 or 4, else ARFLOW_EPARAM), ent [B,2,H,W] of ONE size; per element
 *   of the two channels e = |(pred / n) * n - gt| (n = W, H: the reference's two roundings) goes into bin = the count of
 *   edges[0..nb) <= (double)expf(ent) (np.digitize; edges ascending doubles on the device, 1 <= nb <= 128 else
 *   ARFLOW_EPARAM).  rows [B][arflow_calib_rows(H, W)][nb + 1][3]: count, sum e, sum e^2, in double from the first addition.
 * arflow_uncert_rows / arflow_calib_rows: rows per sample, or ARFLOW_ESHAPE. */
int arflow_uncert_rows(int H, int W);
int arflow_uncert_prep(const float* ent, const float* epe_map, const float* valid, long valid_bstride, float* ent_map,
                       double* rows, float sub_w, float add_W, float sub_h, float add_H, int B, int h, int w, int H, int W,
                       arflow_stream_t stream);
int arflow_sparsify_sums(const float* err, const float* field0, const float* field1, const float* valid,
                         long valid_bstride, const double* thr, float alpha, double* rows, int B, int H, int W, int K,
                         arflow_stream_t stream);
int arflow_calib_rows(int H, int W);
int arflow_calib_hist(const float* pred, const float* gt, const float* ent, const double* edges, double* rows, int B, int C,
                      int H, int W, int nb, arflow_stream_t stream);

/* ---- the rest of the reference's parameter space (no shipped config uses these values; plain kernels) ----------
 * flow_warp(mode='nearest') (utils/warp_utils.py:83-90 -> grid_sample nearest: border clips the coordinate, index =
 * nearbyint, out of range reads 0).  No gradient w.r.t. the flow (grid_sample's nearest mode has none). */
int arflow_warp_nearest_fwd(const float* src, const float* flow, float* out, int B, int C, int Hs, int Ws, int H, int W,
                            long flow_bstride, int pad_mode, int align_corners, int norm_mode, arflow_stream_t stream);
int arflow_warp_nearest_bwd(const float* gout, const float* flow, float* gsrc, int B, int C, int Hs, int Ws, int H, int W,
                            long flow_bstride, int pad_mode, int align_corners, int norm_mode, arflow_stream_t stream);
/* flow_warp(mode='bicubic') (utils/warp_utils.py:83-90 -> grid_sample bicubic, ATen/native/GridSampler.h: A = -0.75, 4 x 4
 * taps at bounded positions, rows first): gradients w.r.t. the source (gsrc, nullable; zero-filled by the call) and the flow
 * (gflow, nullable).  Plain one-thread-per-pixel kernels: no shipped configuration uses this mode. */
int arflow_warp_bicubic_fwd(const float* src, const float* flow, float* out, int B, int C, int Hs, int Ws, int H, int W,
                            long flow_bstride, int pad_mode, int align_corners, int norm_mode, arflow_stream_t stream);
int arflow_warp_bicubic_bwd(const float* gout, const float* src, const float* flow, float* gsrc, float* gflow, int B, int C,
                            int Hs, int Ws, int H, int W, long flow_bstride, int pad_mode, int align_corners, int norm_mode,
                            arflow_stream_t stream);
/* SSIM(x, y, md) distance map of losses/loss_blocks.py:65-84 for any window (2md+1)^2, 1 <= md <= 16:
 * out [B,C,H-2md,W-2md]; arflow_ssim_bwd gives d(sum gmap*out)/dx (call with x and y swapped for d/dy: SSIM is
 * symmetric).  (md = 1 fused with the L1 term and the mask sums is arflow_photo_fwd/bwd.) */
int arflow_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, int md, arflow_stream_t stream);
int arflow_ssim_bwd(const float* x, const float* y, const float* gmap, float* gx, int B, int C, int H, int W, int md,
                    arflow_stream_t stream);
/* arflow_census_fwd / arflow_census_bwd accept 1 <= radius <= 16 (TernaryLoss(max_distance), census_loss(patch_size));
 * radius <= 3 runs the tiled kernels. */
/* Correlation with the CUDA extension's full parameter set (correlation_cuda.cc:10-16, correlation_cuda_kernel.cu:41-114):
 *   out[n, tc, oy, ox] = 1/(K^2 C) sum_{j,i in kernel} sum_c p1[c, y1+j, x1+i] * p2[c, y1+j+tj*s2, x1+i+ti*s2],
 *   p = input zero-padded by pad_size, y1 = oy*stride1 + max_disp, tc = (tj+dr)*(2dr+1)+(ti+dr), dr = max_disp/stride2;
 *   output dims as correlation_cuda.cc:31-34 (arflow_corr_general_out_size).  kernel_size odd.
 * arflow_corr_general_bwd is the exact gradient of that forward (the extension's own backward bounds its window with
 * floor divisions, correlation_cuda_kernel.cu:148-151, and over-counts taps when stride1 > 1).
 * (pad_size = max_disp, kernel_size = stride1 = stride2 = 1 is arflow_corr_fwd/bwd.) */
int arflow_corr_general_out_size(int H, int W, int pad_size, int kernel_size, int max_disp, int stride1, int stride2,
                                 int* out_channels, int* out_h, int* out_w);
int arflow_corr_general_fwd(const float* x1, const float* x2, float* out, int B, int C, int H, int W, int pad_size,
                            int kernel_size, int max_disp, int stride1, int stride2, arflow_stream_t stream);
int arflow_corr_general_bwd(const float* gout, const float* x1, const float* x2, float* gx1, float* gx2, int B, int C, int H,
                            int W, int pad_size, int kernel_size, int max_disp, int stride1, int stride2,
                            arflow_stream_t stream);

/* ---- opt-in bf16 STORAGE of the features ----------------------------------------
 * The reference's native correlation dispatches half-precision tensors as well (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * correlation_cuda_kernel.cu:352,369).  Here: x1 / x2 / src hold bf16 bit patterns (uint16), every product is
 * accumulated in fp32 and every output and gradient is fp32 -- only the bytes read from HBM (and kept for the
 * backward) are halved.  max_disp must be 4.  With negative_slope != 1 the backward takes the LeakyReLU derivative
 * from the sign of the forward output `out`.  Not the default anywhere: callers ask for it explicitly. */
int arflow_corr_fwd_bf16(const unsigned short* x1, const unsigned short* x2, float* out, int B, int C, int H, int W,
                         int max_disp, float negative_slope, arflow_stream_t stream);
int arflow_corr_bwd_bf16(const float* gout, const float* out, const unsigned short* x1, const unsigned short* x2,
                         float* gx1, float* gx2, int B, int C, int H, int W, int max_disp, float negative_slope,
                         arflow_stream_t stream);
int arflow_warp_fwd_bf16(const unsigned short* src, const float* flow, float* out, float* valid, int B, int C, int Hs,
                         int Ws, int H, int W, long flow_bstride, int pad_mode, int align_corners, int norm_mode,
                         arflow_stream_t stream);
int arflow_warp_bwd_bf16(const float* gout, const unsigned short* src, const float* flow, float* gsrc, float* gflow,
                         int B, int C, int Hs, int Ws, int H, int W, long flow_bstride, int pad_mode, int align_corners,
                         int norm_mode, arflow_stream_t stream);

/* ---- on-device batch augmentation (csrc/augment.hip) -------------------------------
 * transforms/geometric_transforms.py:7-15 (crop -> hflip -> scale) and transforms/photometric_transforms.py:7-25 (ColorJitter
 * -> gamma -> channel permutation) on a whole batch:  src [B][F][3][Hs][Ws] contiguous, F = 1 .. ARFLOW_AUG_MAX_FRAMES, dtype
 * ARFLOW_AUG_U8 (0 .. 255, divided by 255) or ARFLOW_AUG_F32 (already in [0,1])  ->  img [B][3F][h][w] (geometric only) and
 * img_ph [B][3F][h][w] (geometric + photometric; NULL: not produced), both float32 and stored from ONE read of src.
 *
 * table: B rows of ARFLOW_AUG_ROW 32-bit words ON THE DEVICE, written once per batch by the host; every frame of a sample
 * uses the sample's row.
 *   word ARFLOW_AUG_Y1, ARFLOW_AUG_X1   int    crop origin in the source (the window is th x tw for every sample; the kernels
 *                                              clamp the origin into [0, Hs - th] x [0, Ws - tw], the HOST checks it)
 *   word ARFLOW_AUG_FLAGS               int    ARFLOW_AUG_FLIP | ARFLOW_AUG_ACTIVE(op) for each active ColorJitter operation |
 *                                              ARFLOW_AUG_GAMMA_ON
 *   word ARFLOW_AUG_ORDER               int    the sample's operation order: the k-th operation applied is bits 2k, 2k + 1
 *                                              (0 brightness, 1 contrast, 2 saturation, 3 hue); inactive ones are skipped
 *   word ARFLOW_AUG_PERM                int    output channel c of every frame is channel (perm >> 2c) & 3 (identity: 0x24)
 *   words ARFLOW_AUG_FACTOR + op        float  the factor of operation op
 *   word ARFLOW_AUG_GAMMA               float  the exponent
 *   the remaining words are reserved (0).
 * scale = 0: (h, w) must equal (th, tw) and img is src / 255 at the mapped pixel bit for bit; scale = 1: the cropped, flipped
 * th x tw image is resized bilinearly to (h, w), align_corners = False.
 *
 * arflow_augment_stats: needed only when some sample has contrast active (and img_ph is wanted).  Stores, for every frame of
 *   such a sample, arflow_augment_partials(h, w) float64 partial sums of grey of the frame as it stands in front of contrast
 *   into work [B F][partials] (one per workgroup; the rows of other samples are not touched and not read).
 * arflow_augment_apply: stores every element of img and, when not NULL, of img_ph; adds a frame's partials in index order.
 *   work may be NULL when no sample has contrast active.  No atomics: two calls give the same bits in either mode.
 * arflow_augment_partials: the partial count per frame, or ARFLOW_ESHAPE; needs no GPU.
 *
 * ARFLOW_ENULL: a required pointer is NULL;  ARFLOW_ESHAPE: B, F, h, w, Hs, Ws, th or tw < 1, F > ARFLOW_AUG_MAX_FRAMES,
 * B F > 65535, a plane of 2^30 elements or more, th > Hs or tw > Ws (a crop window outside the source), (h, w) != (th, tw)
 * with scale = 0;  ARFLOW_EPARAM: dtype or scale not 0 / 1. */
#define ARFLOW_AUG_U8 0
#define ARFLOW_AUG_F32 1
#define ARFLOW_AUG_MAX_FRAMES 5
#define ARFLOW_AUG_ROW 16
#define ARFLOW_AUG_Y1 0
#define ARFLOW_AUG_X1 1
#define ARFLOW_AUG_FLAGS 2
#define ARFLOW_AUG_ORDER 3
#define ARFLOW_AUG_PERM 4
#define ARFLOW_AUG_FACTOR 5
#define ARFLOW_AUG_GAMMA 9
#define ARFLOW_AUG_FLIP 1
#define ARFLOW_AUG_ACTIVE(op) (2 << (op))
#define ARFLOW_AUG_GAMMA_ON 32
int arflow_augment_partials(int h, int w);
int arflow_augment_stats(const void* src, int dtype, const int* table, double* work, int B, int F, int Hs, int Ws, int th,
                         int tw, int h, int w, int scale, arflow_stream_t stream);
int arflow_augment_apply(const void* src, int dtype, const int* table, const double* work, float* img, float* img_ph, int B,
                         int F, int Hs, int Ws, int th, int tw, int h, int w, int scale, arflow_stream_t stream);

/* ---- fused optimiser step on the flat gradient buffer (csrc/optim.hip) --------------
 * trainer/base_trainer.py:78-129 (Adam / the reference's AdamW / SGD over a decay and a no-decay group) and the
 * clip_grad_norm_ of trainer/uflow_elbo_trainer.py:94-99, for the WHOLE model in one launch (two with the norm).
 *
 * grad, s1, s2: flat float32 buffers of n elements in ONE layout (s1 = exp_avg or momentum_buffer, s2 = exp_avg_sq, NULL for
 *   ARFLOW_OPTIM_SGD).  The parameters stay where they are: the chunk table names them.
 * table: nrows rows of ARFLOW_OPTIM_ROW 64-bit words ON THE DEVICE, one workgroup each:
 *   word ARFLOW_OPTIM_ADDR    the address of the row's first parameter element (float32, 4-byte aligned)
 *   word ARFLOW_OPTIM_OFFSET  the flat offset of that element in grad / s1 / s2
 *   word ARFLOW_OPTIM_COUNT   1 .. ARFLOW_OPTIM_CHUNK elements, all of ONE parameter tensor
 *   word ARFLOW_OPTIM_DECAY   the weight decay of the tensor's group, the bits of a double
 *   A row with offset < 0, a count outside 1 .. ARFLOW_OPTIM_CHUNK or offset + count > n is not run.  The kernel cannot check
 *   the address: the caller guarantees it (arflow_amd.optim compares every data_ptr() with the table before every step).
 * arflow_optim_gradnorm: stores arflow_optim_partials(n) float64 partial sums of grad^2 (one per workgroup; no atomics, no
 *   zero-fill: two calls give the same bits in either mode).  arflow_optim_partials needs no GPU; ARFLOW_ESHAPE for n < 1.
 * arflow_optim_step: nparts = 0: no norm, the gradient is used as it stands (clip must be <= 0 and skipped NULL).  nparts =
 *   arflow_optim_partials(n): the partials are added in index order, total_norm = sqrt(sum), and the gradient is multiplied by
 *   min(1, clip / (total_norm + 1e-6)) as it is read when clip > 0 (the stored gradient is NOT rewritten).  skipped != NULL
 *   turns the non-finite guard on: when total_norm is not finite nothing is written but *skipped, which is incremented.
 *   The scalars are doubles and are rounded to float32 once, in the kernel: lr, bc1 = 1 - beta1^t, sqbc2 = sqrt(1 - beta2^t),
 *   eps, beta1 (the momentum for SGD), beta2, clip.  first = 1: SGD's buffer becomes the gradient (its first step).  The
 *   float32 operation order of each rule is written at the head of csrc/optim.hip.
 *
 * ARFLOW_ENULL: a required pointer is NULL;  ARFLOW_ESHAPE: nrows or n < 1, nparts neither 0 nor arflow_optim_partials(n);
 * ARFLOW_EPARAM: an unknown rule, first not 0 / 1, clip > 0 or skipped without partials, lr or clip not finite, a beta outside
 * [0, 1), eps < 0, bc1 or sqbc2 outside (0, 1], a misaligned pointer. */
#define ARFLOW_OPTIM_ADAM 0
#define ARFLOW_OPTIM_ADAMW 1
#define ARFLOW_OPTIM_SGD 2
#define ARFLOW_OPTIM_CHUNK 2048
#define ARFLOW_OPTIM_ROW 4
#define ARFLOW_OPTIM_ADDR 0
#define ARFLOW_OPTIM_OFFSET 1
#define ARFLOW_OPTIM_COUNT 2
#define ARFLOW_OPTIM_DECAY 3
int arflow_optim_partials(long n);
int arflow_optim_gradnorm(const float* grad, double* partials, long n, arflow_stream_t stream);
int arflow_optim_step(const long long* table, int nrows, const float* grad, float* s1, float* s2, long n, const double* partials,
                      int nparts, int* skipped, int rule, int first, double lr, double bc1, double sqbc2, double eps, double beta1,
                      double beta2, double clip, arflow_stream_t stream);

/* ---- the augmentation-regularisation pass (csrc/ar.hip) ----------------------------
 * arflow_ar_transform: ONE launch moves an image stack, a flow field and a non-occlusion mask through a per-sample affine map.
 *   theta [B][6] float32 ON THE DEVICE, (a b tx; c d ty): output pixel (x', y') samples the source position
 *   s = (a x' + b y' + tx, c x' + d y' + ty) in pixel units, bilinear with zero padding (utils/warp_utils.py:83-90 with
 *   pad='zeros', align_corners=True, without grid_sample's normalise / un-normalise round trip).
 *     img [B][C][Hs][Ws]  -> img_t  [B][C][H][W]   every channel of a sample shares its row of theta
 *     flow [B][2][Hs][Ws] -> flow_t [B][2][H][W]   the sampled vector g times the inverse of L = [[a, b], [c, d]]:
 *                                                  u_t = (d g_u - b g_v) / det, v_t = (a g_v - c g_u) / det, det = a d - b c
 *     noc [B][1][Hs][Ws]  -> mask_t [B][1][H][W]   the sampled mask times border_mask (utils/warp_utils.py:119-134, strict:
 *                                                  0 < s_x < Ws - 1 and 0 < s_y < Hs - 1); noc NULL reads as ones
 *   (Hs, Ws) = (H, W) is the reference's flow_warp; another source size carries a ground truth through a crop or a resize.
 *   All tensors dense.  A NULL destination skips its group; a source whose destination is NULL is not read.  The HOST refuses a
 *   row with det = 0 (the kernel divides by it); tap indices are clamped into the plane, so any theta reads inside the planes.
 *   The fp32 operation order is written at the head of csrc/ar.hip.  float4 stores where W % 4 == 0 and the destinations are
 *   16-byte aligned.
 * arflow_ar_loss_fwd: sums[0] = sum over b, c, y, x of (|pred - flow_t| + eps)^q mask, sums[1] = sum over b, y, x of mask, both
 *   float64; pred, flow_t [B][2][H][W], mask [B][1][H][W] or NULL (ones), dense.  One partial pair per workgroup into work
 *   (arflow_ar_loss_partials(B, H, W) pairs of float64; the query needs no GPU), added in index order by a second launch of the
 *   same call.  No atomics, no zero-fill: two calls give the same bits in either mode.
 * arflow_ar_loss_bwd: gpred = (float)gsums[0] q (|e| + eps)^(q - 1) sign(e) mask with e = pred - flow_t and sign(0) = 0, every
 *   element stored; gsums float64 ON THE DEVICE (only gsums[0] is read: there is no gradient to flow_t or mask).
 *
 * ARFLOW_ENULL: theta, pred, flow_t, work, sums, gsums or gpred NULL, or a destination without its source (img_t without img,
 * flow_t without flow);  ARFLOW_ESHAPE: B outside 1 .. 65535, a side (H, W, Hs, Ws) < 1 or > 2^24, a plane of 2^30 elements or more, C < 1
 * with img_t given;  ARFLOW_EPARAM: no destination at all; eps < 0, q <= 0, either not finite, or q < 1 with eps = 0. */
int arflow_ar_transform(const float* theta, const float* img, float* img_t, int C, const float* flow, float* flow_t,
                        const float* noc, float* mask_t, int B, int Hs, int Ws, int H, int W, arflow_stream_t stream);
int arflow_ar_loss_partials(int B, int H, int W);
int arflow_ar_loss_fwd(const float* pred, const float* flow_t, const float* mask, double* work, double* sums, int B, int H,
                       int W, float eps, float q, arflow_stream_t stream);
int arflow_ar_loss_bwd(const float* pred, const float* flow_t, const float* mask, const double* gsums, float* gpred, int B,
                       int H, int W, float eps, float q, arflow_stream_t stream);

/* census_loss_no_penalty (utils/uflow_utils.py:296-306), forward only: ham [B,1,H,W] = the soft census distance of every pixel
 * (the arithmetic of arflow_census_fwd's 32 x 8 kernel: an image compared with itself gives exactly 0), pmask [B,1,H,W] = mask
 * with a border of `radius` pixels zeroed (zero_mask_border).  im_a, im_b [B,3,H,W], mask [B,1,H,W], all dense; any H, W;
 * radius 1 .. 3 (else ARFLOW_EPARAM).  The caller divides pmask by its sum. */
int arflow_census_residual(const float* im_a, const float* im_b, const float* mask, float* ham, float* pmask, int B, int H,
                           int W, int radius, arflow_stream_t stream);

/* ---- EM fit of the Gaussian-mixture penalty and its log-density (csrc/penalty_em.hip) ----
 * train_penalty_em.py:86-220 (class EM) without the m x k responsibility matrix: ONE pass over the samples forms the
 * responsibilities of a sample in registers and keeps four sums per component.
 * arflow_em_stats: x0 [m] samples, float32 (is_f64 = 0) or float64 (1); x1 [m] weights of the same type, or NULL for ones;
 *   logw, beta, mu [k] float64 ON THE DEVICE, 1 <= k <= ARFLOW_EM_KMAX, logw_j = digamma(alpha_bar_j) - digamma(sum alpha_bar) +
 *   log(beta_j) / 2.  In float64 per sample: a_j = -beta_j (x - mu_j)^2 / 2 + logw_j, c = max a, e_j = exp(a_j - c), den = sum e,
 *   xi_j = e_j / den, log xi_j = a_j - c - log(den).  part [arflow_em_partials(m)][4][k] float64, one row per workgroup, every
 *   element stored: S0_j = sum x1 xi_j, S1_j = sum x1 xi_j x, S2_j = sum x1 xi_j (x - mu_j)^2, H_j = sum x1 xi_j log xi_j.
 *   No atomics, no zero-fill: two calls give the same bits in either mode.  Workgroup b takes the samples [b s, (b + 1) s), s a
 *   multiple of ARFLOW_EM_UNIT chosen so that there are at most ARFLOW_EM_MAX_PARTS workgroups.
 * arflow_em_partials: the row count, or ARFLOW_ESHAPE for m < 1; needs no GPU.
 * arflow_em_fold: stats [4][k] = the nparts rows of part added in index order to 0.0.
 * arflow_log_gmm_fwd: out_i = log sum_j w_j exp(-beta_j x_i^2 / 2) as c + log(sum_j w_j exp(arg_j - c)), c = max_j arg_j
 *   (losses/uflow_elbo_loss.py:99-105 with w_j = pi_j sqrt(beta_j) / sqrt(2 pi)); x, out [n] dense, float32 or float64, computed
 *   in that type; w, beta [k] float64 ON THE DEVICE.  arflow_log_gmm_bwd: gx_i = gout_i * -(sum_j r_j beta_j) x_i with r the
 *   posterior weights, recomputed from x.
 *
 * ARFLOW_ENULL: a required pointer is NULL (x1 may be);  ARFLOW_ESHAPE: m or n < 1, nparts outside 1 .. ARFLOW_EM_MAX_PARTS;
 * ARFLOW_EPARAM: k outside 1 .. ARFLOW_EM_KMAX, is_f64 not 0 / 1, a pointer off its element's alignment. */
#define ARFLOW_EM_KMAX 16
#define ARFLOW_EM_UNIT 1024
#define ARFLOW_EM_MAX_PARTS 1024
int arflow_em_partials(long m);
int arflow_em_stats(const void* x0, const void* x1, long m, int is_f64, const double* logw, const double* beta, const double* mu,
                    int k, double* part, arflow_stream_t stream);
int arflow_em_fold(const double* part, int nparts, int k, double* stats, arflow_stream_t stream);
int arflow_log_gmm_fwd(const void* x, long n, int is_f64, const double* w, const double* beta, int k, void* out,
                       arflow_stream_t stream);
int arflow_log_gmm_bwd(const void* x, const void* gout, long n, int is_f64, const double* w, const double* beta, int k, void* gx,
                       arflow_stream_t stream);

/* ---- selectable penalties of UFlowElboLoss (csrc/penalty_dev.hpp) ----------------------------------
 * One pair (rho, rho') per kind, fp32:
 *   ARFLOW_PEN_IDENTITY     rho(x) = x
 *   ARFLOW_PEN_CHARBONNIER  rho(x) = sqrt(x + 1e-6)                       (losses/penalty_functions.py:6-7, eps = 0.001)
 *   ARFLOW_PEN_ABS_ROBUST   rho(x) = (|x| + 0.01)^0.4                     (losses/penalty_functions.py:3-4)
 *   ARFLOW_PEN_GMM          rho(x) = -log sum_j w_j exp(-beta_j x^2 / 2)  data term, x = the soft census distance
 *   ARFLOW_PEN_GMM_SQ       rho(x) = -log sum_j w_j exp(-beta_j x / 2)    smoothness, x = the squared flow difference
 * The mixtures are evaluated in the order of losses/uflow_elbo_loss.py:99-105: arg_j, c = max_j arg_j, e_j = exp(arg_j - c),
 * den = sum_j w_j e_j (j ascending), rho = -(c + log den), rho' = (sum_j w_j e_j beta_j / den) * x (GMM) or / 2 (GMM_SQ).
 * w_j = pi_j sqrt(beta_j) / sqrt(2 pi) is formed by the caller in float64 and rounded to fp32 once, like beta_j.
 * The descriptor lives in HOST memory and is copied into the kernel arguments: no allocation, no synchronisation.
 * Every entry point below answers ARFLOW_ENULL for a NULL descriptor and ARFLOW_EPARAM for an unknown kind, k outside
 * 1 .. ARFLOW_EM_KMAX, a kind it does not take (GMM_SQ in a census call, GMM in a smoothness call), a non-finite or
 * non-positive beta_j, a negative or non-finite w_j, or w = 0 for the component with the smallest beta (its term bounds the
 * density away from 0 for every argument) -- w, beta and k are only read for the two mixture kinds. */
#define ARFLOW_PEN_IDENTITY 0
#define ARFLOW_PEN_CHARBONNIER 1
#define ARFLOW_PEN_ABS_ROBUST 2
#define ARFLOW_PEN_GMM 3
#define ARFLOW_PEN_GMM_SQ 4
typedef struct arflow_penalty_t {
  int kind;
  int k;
  float w[ARFLOW_EM_KMAX];
  float beta[ARFLOW_EM_KMAX];
} arflow_penalty_t;
/* arflow_census_warp_fwd / arflow_census_warp_pair_fwd with the census_loss epilogue rho of `pen` in place of abs_robust_loss:
 * sums numerator = sum rho(ham) pm, dham = pm rho'(ham) -- the plane every census backward entry point reads, so
 * arflow_census_warp_bwd / _pair_bwd serve every kind (the ordered family's too when the environment selects it).
 * valid_flow (nullable; [B,2,H,W] with batch stride valid_bstride >= 2 H W): when given, mask_invalid is taken of THIS flow
 * while the warp still samples at `flow` (occ_type 'mean': the x4 upsample of the mean flow); NULL = `flow`, as today.
 * These two ALWAYS run the column family (csrc/census_col.hpp): ARFLOW_CENSUS_COL / ARFLOW_CENSUS_SYM do not route them.
 * With ARFLOW_PEN_ABS_ROBUST and valid_flow NULL the outputs equal the unpenalised entry points' bit for bit. */
int arflow_census_warp_pen_fwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                               const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H, int W,
                               int radius, const float* valid_flow, long valid_bstride, const arflow_penalty_t* pen,
                               arflow_stream_t stream);
int arflow_census_warp_pair_pen_fwd(const float* gray, const float* flow, long flow_bstride, const float* occ_small,
                                    float* mask_out, float* dham, float* sums, int B2, int H, int W, int radius,
                                    const float* valid_flow, long valid_bstride, const arflow_penalty_t* pen,
                                    arflow_stream_t stream);
/* arflow_census_fwd with a mask and a descriptor, for the unfused route: ham [B,1,H,W] (required: the distances are written
 * there by arflow_census_fwd's kernels, then a second launch applies rho under the border-zeroed mask), dham = pm rho'(ham),
 * sums as arflow_census_fwd.  mask, ham, dham, sums required; radius 1 .. 3 (else ARFLOW_EPARAM); H <= 65535. */
int arflow_census_pen_fwd(const float* im_a, const float* im_b, const float* mask, float* ham, float* dham, float* sums,
                          int B, int H, int W, int radius, const arflow_penalty_t* pen, arflow_stream_t stream);
/* arflow_smooth_fwd / arflow_smooth_bwd with rho of `pen` applied to x = v^2 of the signed (first- or second-order)
 * difference v, d rho / d v = 2 v rho'(x).  Kinds: IDENTITY, CHARBONNIER, ABS_ROBUST, GMM_SQ.  CHARBONNIER is
 * arflow_smooth_fwd / _bwd with penalty = 1 bit for bit.  order, wmode and the edge weights as there. */
int arflow_smooth_pen_fwd(const float* flow, const float* img, float* sums, int B, int Ci, int H, int W, long flow_bstride,
                          float flow_scale, float alpha, int order, int wmode, const arflow_penalty_t* pen,
                          arflow_stream_t stream);
int arflow_smooth_pen_bwd(const float* flow, const float* img, const float* coef, float* gflow, int B, int Ci, int H, int W,
                          long flow_bstride, float flow_scale, float alpha, int order, int wmode, const arflow_penalty_t* pen,
                          arflow_stream_t stream);

/* ---- Flow rendering and original-size restore (csrc/render.hip) ---------------------------------
 * Layouts of a flow argument, and the two output kinds of the render entry points. */
#define ARFLOW_LAYOUT_NCHW 0 /* [B,2,H,W], planes dense, samples flow_bstride floats apart */
#define ARFLOW_LAYOUT_NHWC 1 /* [B,H,W,2], pixels dense, samples flow_bstride floats apart */
#define ARFLOW_RENDER_U8 0   /* uint8, trunc(255 c) of the fp32 product: [B,H,W,3] (flow) / [B,H,W] (scalar) */
#define ARFLOW_RENDER_F32 1  /* float32: [B,3,H,W] planar (flow) / [B,H,W] (scalar) */
#define ARFLOW_RENDER_RGB 0   /* np_flow2rgb, utils/flow_utils.py:84-96 */
#define ARFLOW_RENDER_WHEEL 1 /* flow_to_image, utils/flow_utils.py:67-81 (hsv wheel) */
/* inference.py:98-107 in one pass: flow [B,2,h,w] (samples flow_bstride >= 2 h w floats apart: a channel slice is read in
 * place) -> out_flow [B,H,W,2] dense, the half-pixel bilinear resize (rf_axis of csrc/resize_dev.hpp with align = 0) with
 * u times W / w and v times H / h (the product formed in float64, rounded once).  ent (nullable, same layout rule, stride
 * ent_bstride) -> out_ent [B,H,W,2], the same resize plus 2 log W - 2 log w on channel 0 and 2 log H - 2 log h on channel 1;
 * ent and out_ent are given together or not at all (else ARFLOW_ENULL).  stats (nullable) [B,2]: per sample, over the stored
 * out_flow, (max(|u|, |v|), max(u, v)); integer atomic maxima on the float bits, so the result does not depend on the order
 * (bitwise repeatable, allowed in deterministic mode).  A NaN in the flow leaves its sample's stats unspecified.
 * Launches: one kernel; with stats, a B-lane kernel in front of it that stores the identities (0, -inf). */
int arflow_restore_out(const float* flow, long flow_bstride, const float* ent, long ent_bstride, float* out_flow,
                       float* out_ent, float* stats, int B, int h, int w, int H, int W, arflow_stream_t stream);
/* the same stats [B,2] of a flow that is already at its final size, in either layout */
int arflow_flow_stats(const float* flow, long flow_bstride, int layout, float* stats, int B, int H, int W,
                      arflow_stream_t stream);
/* flow -> colour.  scale: sample b is normalised by scale[b * scale_stride] (so scale may point at either column of stats
 * with scale_stride = 2); a scale that is not positive and finite renders white (normalised flow 0 / saturation 0).
 * mode RGB: n = f / scale, (1 + n_u, 1 - 0.5 (n_u + n_v), 1 + n_v) clipped to [0,1], the reference's fp32 sequence.
 * mode WHEEL: h = mod(atan2(v,u) / 2 pi + 1, 1), s = clip(8 |f| / scale), val = clip(8 - s), matplotlib's hsv_to_rgb.
 * out: uint8 [B,H,W,3] (ARFLOW_RENDER_U8) or float [B,3,H,W] (ARFLOW_RENDER_F32), dense. */
int arflow_flow_render(const float* flow, long flow_bstride, int layout, const float* scale, int scale_stride, void* out,
                       int out_kind, int mode, int B, int H, int W, arflow_stream_t stream);
/* uflow_elbo_trainer.py:259-262: e = sum over the C (1 .. 16) channels of x [B,C,H,W] (samples x_bstride floats apart), added
 * in channel order.  arflow_scalar_stats: minmax [2] = (min e, max e) over the WHOLE batch (atomics as above, identities
 * stored by a one-lane kernel in front).  arflow_scalar_render: (e - min) / (max - min) as float or trunc(255 .) uint8
 * [B,H,W]; max == min (a constant map) renders 0. */
int arflow_scalar_stats(const float* x, long x_bstride, int C, float* minmax, int B, int H, int W, arflow_stream_t stream);
int arflow_scalar_render(const float* x, long x_bstride, int C, const float* minmax, void* out, int out_kind, int B, int H,
                         int W, arflow_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARFLOW_HIP_H */
