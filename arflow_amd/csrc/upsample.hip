// The bilinear upsamples and their gather adjoints, built from upsample_dev.hpp:
//
//   out[b,c] = s_c * upsample_bilinear2d(in[b,c] + b_c, x f, align_corners),  s_c = f for c < n_flow else 1,
//                                                          b_c = diag_bias for n_flow <= c < n_flow + n_diag else 0
//
//   flow_up   f = 2, 4, either align flag, C = n_flow = 2, no bias add, dense [B,2,h,w]: F.interpolate(flow * f, scale_factor=f)
//             as the reference models bring a flow to the next level or to full resolution (models/pwclite.py:54,66,92,104;
//             models/pwclite_uflow.py:104,124; utils/uflow_utils.py:163-180 upsample(is_flow)); DESIGN.md section 14
//   out_up2   f = 2, align_corners=False: models/uflow_prob_model.py:223-250 upsample_out -- the output split into (flow,
//             log_diag, rest), each group resized with its own affine rule, concatenated -- as one launch over all channels,
//             and the model's last two calls (level 2 -> level 1 -> level 0) as one launch that reads the level-2 tensor
//             once (out_tail); DESIGN.md section 22
//   prob_up   f = 2, 4, align_corners=True: models/pwclite_prob.py:183-186,216-217; DESIGN.md section 27
//   up2_bwd   the adjoint of the x2 flow upsample inside the fused level (up2_source in warp.hip / level_small.hip)
//
// Every adjoint is a gather, one thread per coarse cell, rows ascending and columns ascending inside a row (ATen's backward
// of the resize scatters with float atomics): reproducible in either mode.  The bias has no gradient.  Planes are contiguous
// (h*w floats between channels); where an entry point takes batch strides a source can be a channel slice of a wider tensor
// and a destination a slot of a concatenated buffer.
#include "common.hpp"
#include "level_internal.hpp"
#include "upsample_dev.hpp"

namespace {
// Forward: V fine pixels of one row per thread (V = 4: one float4 store per lane; V = 1: odd widths / unaligned slots).
template <int V, bool BIAS>
__global__ __launch_bounds__(256) void up_fwd_kernel(const float* __restrict__ in, long in_bs, float* __restrict__ out, long out_bs,
                                                     int B, int C, int h, int w, int f, float rs, int align, int n_flow,
                                                     int n_diag, float diag_bias) {
  const int H = f * h, W = f * w, Wq = W / V;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * H * Wq) return;
  const int xq = (int)(idx % Wq), y = (int)((idx / Wq) % H);
  const long pl = idx / ((long)Wq * H);
  const int c = (int)(pl % C), b = (int)(pl / C);
  float sc, bias;
  up_chan_rule(c, n_flow, n_diag, diag_bias, f, sc, bias);
  up_fwd_group<V, BIAS>(in + (long)b * in_bs + (long)c * h * w, out + (long)b * out_bs + ((long)c * H + y) * W, y, xq * V, h, w,
                        H, W, rs, align != 0, sc, bias);
}

// Adjoint of the x2 flow upsample of the level forward, times the factor 2 of interpolate(flow * 2): rows 2i-2 .. 2i+3 cover
// either align flag; a row or column outside the image is read at the clamped index with weight 0 (no branch in the 36
// unrolled taps).  The hot path's kernel (second launch of every fused level backward): dense planes, one scale, and the
// body as it was in warp.hip -- as an instance of up_gather_static it compiled to another register allocation.
__global__ __launch_bounds__(256) void up2_bwd_kernel(const float* __restrict__ gfine, float* __restrict__ gcoarse,
                                                      int planes, int H, int W, int up_align) {
  const int Hc = H / 2, Wc = W / 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)planes * Hc * Wc) return;
  const int j = (int)(idx % Wc), i = (int)((idx / Wc) % Hc);
  const long pl = idx / ((long)Wc * Hc);
  const float* g = gfine + pl * H * W;
  float wy[6], wx[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int y = 2 * i - 2 + k;
    wy[k] = 0.f;
    if (y >= 0 && y < H) wy[k] = up_weight(y, i, Hc, H, 0.5f, up_align != 0);
    const int x = 2 * j - 2 + k;
    wx[k] = 0.f;
    if (x >= 0 && x < W) wx[k] = up_weight(x, j, Wc, W, 0.5f, up_align != 0);
  }
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < 6; ++ky) {
    const int y = min(max(2 * i - 2 + ky, 0), H - 1);
    float row = 0.f;
#pragma unroll
    for (int kx = 0; kx < 6; ++kx) {
      const int x = min(max(2 * j - 2 + kx, 0), W - 1);
      row = fmaf(wx[kx], g[(long)y * W + x], row);
    }
    acc = fmaf(wy[ky], row, acc);
  }
  gcoarse[idx] = 2.f * acc;
}

// ... of the x2 output upsample (align_corners=False): fine row y reads coarse rows floor((y - 0.5) / 2) and the next, so
// coarse row i is read by fine rows 2i - 1 .. 2i + 2 -- at most 4 x 4 fine pixels; those outside the image are skipped.
__global__ __launch_bounds__(256) void out_up2_bwd_kernel(const float* __restrict__ gfine, long gf_bs, float* __restrict__ gcoarse,
                                                          long gc_bs, int B, int C, int h, int w, int n_flow) {
  const int H = 2 * h, W = 2 * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * h * w) return;
  const int j = (int)(idx % w), i = (int)((idx / w) % h);
  const long pl = idx / ((long)w * h);
  const int c = (int)(pl % C), b = (int)(pl / C);
  const float* g = gfine + (long)b * gf_bs + (long)c * H * W;
  gcoarse[(long)b * gc_bs + ((long)c * h + i) * w + j] =
      up_chan_scale(c, n_flow, 2) * up_gather_static<4>(g, i, j, 2 * i - 1, 2 * j - 1, h, w, H, W, false);
}

// ... of any factor, over fine_run's rows and columns.  The align flag at compile time: the source map's branch sits in
// the innermost loops.
template <bool ALIGN>
__global__ __launch_bounds__(256) void up_run_bwd_kernel(const float* __restrict__ gfine, long gf_bs, float* __restrict__ gcoarse,
                                                         long gc_bs, int B, int C, int h, int w, int f, int n_flow) {
  const int H = f * h, W = f * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * h * w) return;
  const int j = (int)(idx % w), i = (int)((idx / w) % h);
  const long pl = idx / ((long)w * h);
  const int c = (int)(pl % C), b = (int)(pl / C);
  const float* g = gfine + (long)b * gf_bs + (long)c * H * W;
  gcoarse[(long)b * gc_bs + ((long)c * h + i) * w + j] =
      up_chan_scale(c, n_flow, f) * up_gather_run(g, i, j, h, w, H, W, f, ALIGN ? 0.f : 1.f / (float)f, ALIGN);
}

// ---- the model's tail: level 2 -> level 1 -> level 0 in one launch ---------------------------------------------------
// One workgroup = one TAIL_TH x TAIL_TW tile of one level-2 plane.  s2: the tile with a one-cell halo, bias already added.
// s1: the level-1 tile (2 TH x 2 TW) with ITS one-cell halo, as the rounded fp32 values a x2 launch would have stored --
// level 0 is computed from those, so out0 is bit for bit what a second launch computes from the stored out1.
// s1's row pitch is odd (35): in the level-0 pass lane l of a wave handles four pixels of fine row r0 + l / 16 at columns
// 4 (l % 16) .., i.e. reads s1 columns 2 (l % 16) - 1 + k: a stride of two dwords along a row.  ds_read_b32 serves lanes
// 0-31 and 32-63 as two groups over 32 banks; a group holds two fine rows whose taps lie in two adjacent s1 rows (or the
// same one: equal addresses broadcast), and with an odd pitch those two rows use the even and the odd banks: no conflict.
constexpr int TAIL_TH = 8, TAIL_TW = 16;
constexpr int S2H = TAIL_TH + 2, S2W = TAIL_TW + 2;
constexpr int S1H = 2 * TAIL_TH + 2, S1W = 2 * TAIL_TW + 2, S1P = S1W + 1;

template <bool VEC>
__global__ __launch_bounds__(256) void out_tail_fwd_kernel(const float* __restrict__ in, long in_bs, float* __restrict__ out1,
                                                           float* __restrict__ out0, int B, int C, int h, int w, int n_flow,
                                                           int n_diag, float diag_bias, int ntx, int nty) {
  __shared__ float s2[S2H * S2W];
  __shared__ float s1[S1H * S1P];
  int tx, ty, pl;
  if (!af_tile_of_block(ntx, nty, B * C, tx, ty, pl)) return;
  const int c = pl % C, b = pl / C;
  float sc, bias;
  up_chan_rule(c, n_flow, n_diag, diag_bias, 2, sc, bias);
  const int h1 = 2 * h, w1 = 2 * w, h0 = 4 * h, w0 = 4 * w;
  const int y2 = ty * TAIL_TH - 1, x2 = tx * TAIL_TW - 1;          // level-2 coordinates of s2[0]
  const int y1 = 2 * ty * TAIL_TH - 1, x1 = 2 * tx * TAIL_TW - 1;  // level-1 coordinates of s1[0]
  const float* src = in + (long)b * in_bs + (long)c * h * w;
  // cells outside the image hold the clamped neighbour: every index up_source returns is clamped into the image, so
  // whatever a level-1 cell inside the image asks for is present
  for (int i = threadIdx.x; i < S2H * S2W; i += 256) {
    const int r = i / S2W, q = i % S2W;
    const int gy = min(max(y2 + r, 0), h - 1), gx = min(max(x2 + q, 0), w - 1);
    s2[i] = src[(long)gy * w + gx] + bias;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S1H * S1W; i += 256) {
    const int r = i / S1W, q = i % S1W;
    const int gy = y1 + r, gx = x1 + q;
    if (gy < 0 || gy >= h1 || gx < 0 || gx >= w1) continue;  // never read: level 0 asks for clamped indices only
    int ya, yb, xa, xb;
    float wy0, wy1, wx0, wx1;
    up_source(gy, h, h1, 0.5f, false, ya, yb, wy0, wy1);
    up_source(gx, w, w1, 0.5f, false, xa, xb, wx0, wx1);
    const float* ra = s2 + (ya - y2) * S2W - x2;
    const float* rb = s2 + (yb - y2) * S2W - x2;
    s1[r * S1P + q] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa], ra[xb], rb[xa], rb[xb]);
  }
  __syncthreads();
  // level 1: the tile's interior
  float* o1 = out1 + (long)pl * h1 * w1;
  if constexpr (VEC) {
    for (int i = threadIdx.x; i < 2 * TAIL_TH * (2 * TAIL_TW / 4); i += 256) {
      const int r = i / (2 * TAIL_TW / 4), q = 4 * (i % (2 * TAIL_TW / 4));
      const int gy = y1 + 1 + r, gx = x1 + 1 + q;
      if (gy >= h1 || gx >= w1) continue;  // w1 % 4 == 0: a group of four is inside or outside as a whole
      const float* p = s1 + (r + 1) * S1P + q + 1;
      *reinterpret_cast<float4*>(o1 + (long)gy * w1 + gx) = make_float4(p[0], p[1], p[2], p[3]);
    }
  } else {
    for (int i = threadIdx.x; i < 2 * TAIL_TH * 2 * TAIL_TW; i += 256) {
      const int r = i / (2 * TAIL_TW), q = i % (2 * TAIL_TW);
      const int gy = y1 + 1 + r, gx = x1 + 1 + q;
      if (gy >= h1 || gx >= w1) continue;
      o1[(long)gy * w1 + gx] = s1[(r + 1) * S1P + q + 1];
    }
  }
  // level 0 from the level-1 values in LDS: four pixels of one row per lane (w0 = 4 w: always whole groups of four)
  float* o0 = out0 + (long)pl * h0 * w0;
  for (int i = threadIdx.x; i < 4 * TAIL_TH * TAIL_TW; i += 256) {
    const int r = i / TAIL_TW, q = 4 * (i % TAIL_TW);
    const int gy = 4 * ty * TAIL_TH + r, gx = 4 * tx * TAIL_TW + q;
    if (gy >= h0 || gx >= w0) continue;
    int ya, yb;
    float wy0, wy1;
    up_source(gy, h1, h0, 0.5f, false, ya, yb, wy0, wy1);
    const float* ra = s1 + (ya - y1) * S1P - x1;
    const float* rb = s1 + (yb - y1) * S1P - x1;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int xa, xb;
      float wx0, wx1;
      up_source(gx + k, w1, w0, 0.5f, false, xa, xb, wx0, wx1);
      v[k] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa] + bias, ra[xb] + bias, rb[xa] + bias, rb[xb] + bias);
    }
    float* o = o0 + (long)gy * w0 + gx;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    }
  }
}

// The argument check of every entry point: a [B,C,h,w] coarse tensor with h, w <= max_hw, a fine one a_scale / o_scale times
// its size on the input / output side (scale 0: a dense tensor, no stride to check).
int up_check(const void* a, long a_bs, const void* o, long o_bs, int B, int C, int h, int w, int max_hw, int n_flow, int n_diag,
             int a_scale, int o_scale) {
  AF_REQUIRE_PTR(a);
  AF_REQUIRE_PTR(o);
  AF_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && B <= 65535 && C <= 65535 && h <= max_hw && w <= max_hw, ARFLOW_ESHAPE);
  AF_REQUIRE((long)B * C <= (1L << 24), ARFLOW_ESHAPE);
  AF_REQUIRE(n_flow >= 0 && n_diag >= 0 && n_flow + n_diag <= C, ARFLOW_EPARAM);
  const long plane = (long)C * h * w;
  AF_REQUIRE(B == 1 || (a_bs >= plane * a_scale && o_bs >= plane * o_scale), ARFLOW_ESHAPE);
  return ARFLOW_OK;
}

// One thread per item, 256 per workgroup.
template <class... P, class... A>
int up_launch(void (*kernel)(P...), long n, hipStream_t st, A... args) {
  kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(args...);
  return af_launch_status();
}

// Forward: four pixels per thread where a fine row is whole float4 groups and every item starts on one, else one.
template <bool BIAS>
int up_fwd_launch(const float* in, long in_bs, float* out, long out_bs, int B, int C, int h, int w, int f, int align, int n_flow,
                  int n_diag, float diag_bias, hipStream_t st) {
  const long n = (long)B * C * f * f * h * w;
  const float rs = 1.f / (float)f;  // exact
  if (((long)f * w) % 4 == 0 && af_vec4_ok(out, out_bs, B))
    return up_launch(up_fwd_kernel<4, BIAS>, n / 4, st, in, in_bs, out, out_bs, B, C, h, w, f, rs, align, n_flow, n_diag, diag_bias);
  return up_launch(up_fwd_kernel<1, BIAS>, n, st, in, in_bs, out, out_bs, B, C, h, w, f, rs, align, n_flow, n_diag, diag_bias);
}

// Adjoint over fine_run (any factor); the x2 entry points name their static window themselves.
int up_run_bwd_launch(const float* gfine, long gf_bs, float* gcoarse, long gc_bs, int B, int C, int h, int w, int f, int align,
                      int n_flow, hipStream_t st) {
  return up_launch(align ? up_run_bwd_kernel<true> : up_run_bwd_kernel<false>, (long)B * C * h * w, st, gfine, gf_bs, gcoarse,
                   gc_bs, B, C, h, w, f, n_flow);
}
}  // namespace

int af_up2_bwd_launch(const float* gfine, float* gcoarse, int planes, int H, int W, int up_align, hipStream_t st) {
  return up_launch(up2_bwd_kernel, (long)planes * (H / 2) * (W / 2), st, gfine, gcoarse, planes, H, W, up_align);
}

// Adjoint of `flow_up = interpolate(flow * 2, x2, bilinear)` as arflow_level_warp_fwd evaluates it (gather form, no
// atomics, gcoarse fully written): gfine [B,2,H,W] -> gcoarse [B,2,H/2,W/2].  models/pwclite.py:178-179 backward.
extern "C" int arflow_up2_bwd(const float* gfine, float* gcoarse, int B, int H, int W, int up_align_corners,
                              arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = up_check(gfine, 0, gcoarse, 0, B, 2, H / 2, W / 2, 1 << 30, 2, 0, 0, 0);  // dense: no stride to check
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(H % 2 == 0 && W % 2 == 0, ARFLOW_ESHAPE);
  return af_up2_bwd_launch(gfine, gcoarse, B * 2, H, W, up_align_corners, (hipStream_t)stream);
}

extern "C" int arflow_flow_up_fwd(const float* flow, float* out, int B, int h, int w, int factor, int align_corners,
                                  arflow_stream_t stream) {
  af_clear_stale_error();
  const long plane = 2L * h * w;
  const int rc = up_check(flow, 0, out, 0, B, 2, h, w, 16384, 2, 0, 0, 0);  // dense: no stride to check
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  return up_fwd_launch<false>(flow, plane, out, plane * factor * factor, B, 2, h, w, factor, align_corners, 2, 0, 0.f,
                              (hipStream_t)stream);
}

// (factor 2: the level's 6 x 6 window, which lies inside fine_run's)
extern "C" int arflow_flow_up_bwd(const float* gfine, float* gcoarse, int B, int h, int w, int factor, int align_corners,
                                  arflow_stream_t stream) {
  af_clear_stale_error();
  const long plane = 2L * h * w;
  const int rc = up_check(gfine, 0, gcoarse, 0, B, 2, h, w, 16384, 2, 0, 0, 0);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  if (factor == 2) return af_up2_bwd_launch(gfine, gcoarse, B * 2, 2 * h, 2 * w, align_corners, (hipStream_t)stream);
  return up_run_bwd_launch(gfine, plane * factor * factor, gcoarse, plane, B, 2, h, w, factor, align_corners, 2,
                           (hipStream_t)stream);
}

extern "C" int arflow_out_up2_fwd(const float* in, long in_bstride, float* out, long out_bstride, int B, int C, int h, int w,
                                  int n_flow, int n_diag, float diag_bias, arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = up_check(in, in_bstride, out, out_bstride, B, C, h, w, 8192, n_flow, n_diag, 1, 4);
  if (rc != ARFLOW_OK) return rc;
  return up_fwd_launch<true>(in, in_bstride, out, out_bstride, B, C, h, w, 2, 0, n_flow, n_diag, diag_bias, (hipStream_t)stream);
}

extern "C" int arflow_out_up2_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C,
                                  int h, int w, int n_flow, arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = up_check(gfine, gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, 8192, n_flow, 0, 4, 1);
  if (rc != ARFLOW_OK) return rc;
  return up_launch(out_up2_bwd_kernel, (long)B * C * h * w, (hipStream_t)stream, gfine, gfine_bstride, gcoarse, gcoarse_bstride,
                   B, C, h, w, n_flow);
}

extern "C" int arflow_out_tail_fwd(const float* in, long in_bstride, float* out1, float* out0, int B, int C, int h, int w,
                                   int n_flow, int n_diag, float diag_bias, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(out0);
  const int rc = up_check(in, in_bstride, out1, (long)C * 4 * h * w, B, C, h, w, 8192, n_flow, n_diag, 1, 4);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(h <= 4096 && w <= 4096, ARFLOW_ESHAPE);
  const int ntx = af_cdiv(w, TAIL_TW), nty = af_cdiv(h, TAIL_TH);
  const long T = (long)ntx * nty * B * C;
  AF_REQUIRE(T <= (1L << 30), ARFLOW_ESHAPE);
  const dim3 grid(af_grid_for_tiles(T));
  if (w % 2 == 0 && af_aligned16(out1) && af_aligned16(out0)) {
    hipLaunchKernelGGL(out_tail_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, in_bstride, out1, out0, B, C, h,
                       w, n_flow, n_diag, diag_bias, ntx, nty);
  } else {
    hipLaunchKernelGGL(out_tail_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, in_bstride, out1, out0, B, C,
                       h, w, n_flow, n_diag, diag_bias, ntx, nty);
  }
  return af_launch_status();
}

extern "C" int arflow_prob_up_fwd(const float* in, long in_bstride, float* out, long out_bstride, int B, int C, int h, int w,
                                  int factor, int n_flow, int n_diag, float diag_bias, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  const int rc = up_check(in, in_bstride, out, out_bstride, B, C, h, w, 8192, n_flow, n_diag, 1, factor * factor);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(h <= 2048 && w <= 2048, ARFLOW_ESHAPE);
  return up_fwd_launch<true>(in, in_bstride, out, out_bstride, B, C, h, w, factor, 1, n_flow, n_diag, diag_bias,
                             (hipStream_t)stream);
}

extern "C" int arflow_prob_up_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C,
                                  int h, int w, int factor, int n_flow, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  const int rc = up_check(gfine, gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, 8192, n_flow, 0, factor * factor, 1);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(h <= 2048 && w <= 2048, ARFLOW_ESHAPE);
  return up_run_bwd_launch(gfine, gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, factor, 1, n_flow, (hipStream_t)stream);
}
