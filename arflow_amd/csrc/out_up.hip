// Output upsample of the probabilistic PWC model: models/uflow_prob_model.py:223-250 upsample_out --
// split the output into (flow, log_diag, rest), upsample each group x2 bilinear (align_corners=False) with its own affine
// rule (flow: times 2; log_diag: + diag_bias BEFORE the resize; rest: plain) and concatenate -- as one launch over all
// channels, with a gather adjoint (no atomics: ATen's backward of the resize scatters), and the model's last two calls
// (level 2 -> level 1 -> level 0) as one launch that reads the level-2 tensor once.
//
//   out[b,c] = s_c * upsample_bilinear2d(in[b,c] + b_c),  s_c = 2 for c < n_flow else 1,
//                                                          b_c = diag_bias for n_flow <= c < n_flow + n_diag else 0
//
// The index / weight arithmetic is up_source / up_blend (taps.hpp), the same device code as flow_up.hip and the fused
// level's x2 case.  Planes are contiguous (h*w floats between channels); every tensor has its own batch stride, so a
// source can be a channel slice of a wider tensor and a destination a slot of a concatenated buffer.
#include "common.hpp"
#include "taps.hpp"

namespace {
__device__ __forceinline__ void chan_rule(int c, int n_flow, int n_diag, float diag_bias, float& s, float& b) {
  s = c < n_flow ? 2.f : 1.f;
  b = (c >= n_flow && c < n_flow + n_diag) ? diag_bias : 0.f;
}

// V fine pixels of one row per thread (V = 4: one float4 store per lane; V = 1: odd widths / unaligned slots).  The bias
// is added on load (a + 0 is a for the other channels), the power-of-two scale after the blend: the reference's order.
template <int V>
__global__ __launch_bounds__(256) void out_up2_fwd_kernel(const float* __restrict__ in, long in_bs, float* __restrict__ out,
                                                          long out_bs, int B, int C, int h, int w, int n_flow, int n_diag,
                                                          float diag_bias) {
  const int H = 2 * h, W = 2 * w, Wq = W / V;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * H * Wq) return;
  const int xq = (int)(idx % Wq), y = (int)((idx / Wq) % H);
  const long pl = idx / ((long)Wq * H);
  const int c = (int)(pl % C), b = (int)(pl / C);
  float sc, bias;
  chan_rule(c, n_flow, n_diag, diag_bias, sc, bias);
  int ya, yb;
  float wy0, wy1;
  up_source(y, h, H, 0.5f, false, ya, yb, wy0, wy1);
  const float* s = in + (long)b * in_bs + (long)c * h * w;
  const float* ra = s + (long)ya * w;
  const float* rb = s + (long)yb * w;
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int xa, xb;
    float wx0, wx1;
    up_source(xq * V + k, w, W, 0.5f, false, xa, xb, wx0, wx1);
    r[k] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa] + bias, ra[xb] + bias, rb[xa] + bias, rb[xb] + bias);
  }
  float* o = out + (long)b * out_bs + ((long)c * H + y) * W + xq * V;
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    o[0] = r[0];
  }
}

// Adjoint as a gather: one thread per coarse cell (i, j).  With scale 2 and align_corners=False fine row y reads coarse rows
// floor((y - 0.5) / 2) and the next, so coarse row i is read by fine rows 2i - 1 .. 2i + 2 (clamped to the image; at the
// image border both clamped taps of a fine row can be row i, then their weights add) -- at most 4 x 4 fine pixels, rows
// ascending, columns ascending inside a row.  The weights themselves come from up_source.  The bias has no gradient.
__global__ __launch_bounds__(256) void out_up2_bwd_kernel(const float* __restrict__ gfine, long gf_bs, float* __restrict__ gcoarse,
                                                          long gc_bs, int B, int C, int h, int w, int n_flow) {
  const int H = 2 * h, W = 2 * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * h * w) return;
  const int j = (int)(idx % w), i = (int)((idx / w) % h);
  const long pl = idx / ((long)w * h);
  const int c = (int)(pl % C), b = (int)(pl / C);
  const float* g = gfine + (long)b * gf_bs + (long)c * H * W;
  // the four column weights once per cell (a column outside the image is skipped, not read)
  float wx[4];
  bool vx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = 2 * j - 1 + k;
    vx[k] = x >= 0 && x < W;
    int a0, a1;
    float l0, l1;
    up_source(vx[k] ? x : 0, w, W, 0.5f, false, a0, a1, l0, l1);
    wx[k] = (a0 == j ? l0 : 0.f) + (a1 == j ? l1 : 0.f);
  }
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = 2 * i - 1 + r;
    if (y < 0 || y >= H) continue;
    int a0, a1;
    float l0, l1;
    up_source(y, h, H, 0.5f, false, a0, a1, l0, l1);
    const float wy = (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
    const float* gr = g + (long)y * W + (2 * j - 1);
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (vx[k]) row = fmaf(wx[k], gr[k], row);
    acc = fmaf(wy, row, acc);
  }
  gcoarse[(long)b * gc_bs + ((long)c * h + i) * w + j] = (c < n_flow ? 2.f : 1.f) * acc;
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
  chan_rule(c, n_flow, n_diag, diag_bias, sc, bias);
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

// ---- the align_corners=True sibling for factors 2 and 4: models/pwclite_prob.py:183-186,216-217 ------
//   out[b,c] = s_c * upsample_bilinear2d(in[b,c] + b_c, x f, align_corners=True),  s_c = f for c < n_flow else 1
// Source index and weights: up_source's align branch (scale = (h - 1) / (H - 1) in fp32, src = scale * dst: ATen's order).
template <int V>
__global__ __launch_bounds__(256) void prob_up_fwd_kernel(const float* __restrict__ in, long in_bs, float* __restrict__ out,
                                                          long out_bs, int B, int C, int h, int w, int f, int n_flow, int n_diag,
                                                          float diag_bias) {
  const int H = f * h, W = f * w, Wq = W / V;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * H * Wq) return;
  const int xq = (int)(idx % Wq), y = (int)((idx / Wq) % H);
  const long pl = idx / ((long)Wq * H);
  const int c = (int)(pl % C), b = (int)(pl / C);
  const float sc = c < n_flow ? (float)f : 1.f;  // chan_rule with the factor in place of 2
  const float bias = (c >= n_flow && c < n_flow + n_diag) ? diag_bias : 0.f;
  int ya, yb;
  float wy0, wy1;
  up_source(y, h, H, 0.f, true, ya, yb, wy0, wy1);
  const float* s = in + (long)b * in_bs + (long)c * h * w;
  const float* ra = s + (long)ya * w;
  const float* rb = s + (long)yb * w;
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int xa, xb;
    float wx0, wx1;
    up_source(xq * V + k, w, W, 0.f, true, xa, xb, wx0, wx1);
    r[k] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa] + bias, ra[xb] + bias, rb[xa] + bias, rb[xb] + bias);
  }
  float* o = out + (long)b * out_bs + ((long)c * H + y) * W + xq * V;
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    o[0] = r[0];
  }
}

// Adjoint as a gather: one thread per coarse cell over fine_run's rows and columns (taps.hpp; the run is generous, a fine
// pixel that does not read the cell weighs 0), rows ascending, columns ascending inside a row.  The bias has no gradient.
// The column weights are the same for every row: the first PROB_UP_COLS of the run are computed once and kept in registers
// (for factors 2 and 4 the run is at most 2 * 5 + 5 = 15 columns wide once w >= 4, and at most W <= 12 below that); columns
// beyond them, should a run ever be wider, are weighed where they are used.  Same weights, same order of additions.
constexpr int PROB_UP_COLS = 16;
__global__ __launch_bounds__(256) void prob_up_bwd_kernel(const float* __restrict__ gfine, long gf_bs, float* __restrict__ gcoarse,
                                                          long gc_bs, int B, int C, int h, int w, int f, int n_flow) {
  const int H = f * h, W = f * w;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C * h * w) return;
  const int j = (int)(idx % w), i = (int)((idx / w) % h);
  const long pl = idx / ((long)w * h);
  const int c = (int)(pl % C), b = (int)(pl / C);
  const float* g = gfine + (long)b * gf_bs + (long)c * H * W;
  int ylo, yhi, xlo, xhi;
  fine_run(i, h, H, f, true, ylo, yhi);
  fine_run(j, w, W, f, true, xlo, xhi);
  float wx[PROB_UP_COLS];
#pragma unroll
  for (int k = 0; k < PROB_UP_COLS; ++k) {
    int a0, a1;
    float l0, l1;
    up_source(min(xlo + k, W - 1), w, W, 0.f, true, a0, a1, l0, l1);
    wx[k] = (a0 == j ? l0 : 0.f) + (a1 == j ? l1 : 0.f);
  }
  float acc = 0.f;
  for (int y = ylo; y <= yhi; ++y) {
    int a0, a1;
    float l0, l1;
    up_source(y, h, H, 0.f, true, a0, a1, l0, l1);
    const float wy = (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
    const float* gr = g + (long)y * W;
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < PROB_UP_COLS; ++k)
      if (xlo + k <= xhi) row = fmaf(wx[k], gr[xlo + k], row);
    for (int x = xlo + PROB_UP_COLS; x <= xhi; ++x) {
      up_source(x, w, W, 0.f, true, a0, a1, l0, l1);
      row = fmaf((a0 == j ? l0 : 0.f) + (a1 == j ? l1 : 0.f), gr[x], row);
    }
    acc = fmaf(wy, row, acc);
  }
  gcoarse[(long)b * gc_bs + ((long)c * h + i) * w + j] = (c < n_flow ? (float)f : 1.f) * acc;
}

int out_up_check(const void* a, long a_bs, const void* o, long o_bs, int B, int C, int h, int w, int n_flow, int n_diag,
                 int a_scale, int o_scale) {
  AF_REQUIRE_PTR(a);
  AF_REQUIRE_PTR(o);
  AF_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && B <= 65535 && C <= 65535 && h <= 8192 && w <= 8192, ARFLOW_ESHAPE);
  AF_REQUIRE((long)B * C <= (1L << 24), ARFLOW_ESHAPE);
  AF_REQUIRE(n_flow >= 0 && n_diag >= 0 && n_flow + n_diag <= C, ARFLOW_EPARAM);
  const long plane = (long)C * h * w;
  AF_REQUIRE(B == 1 || (a_bs >= plane * a_scale && o_bs >= plane * o_scale), ARFLOW_ESHAPE);
  return ARFLOW_OK;
}
}  // namespace

extern "C" int arflow_out_up2_fwd(const float* in, long in_bstride, float* out, long out_bstride, int B, int C, int h, int w,
                                  int n_flow, int n_diag, float diag_bias, arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = out_up_check(in, in_bstride, out, out_bstride, B, C, h, w, n_flow, n_diag, 1, 4);
  if (rc != ARFLOW_OK) return rc;
  const long n = (long)B * C * 4 * h * w;
  if (w % 2 == 0 && af_vec4_ok(out, out_bstride, B)) {
    hipLaunchKernelGGL(out_up2_fwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                       in_bstride, out, out_bstride, B, C, h, w, n_flow, n_diag, diag_bias);
  } else {
    hipLaunchKernelGGL(out_up2_fwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                       in_bstride, out, out_bstride, B, C, h, w, n_flow, n_diag, diag_bias);
  }
  return af_launch_status();
}

extern "C" int arflow_out_up2_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C,
                                  int h, int w, int n_flow, arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = out_up_check(gfine, gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, n_flow, 0, 4, 1);
  if (rc != ARFLOW_OK) return rc;
  const long n = (long)B * C * h * w;
  hipLaunchKernelGGL(out_up2_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gfine,
                     gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, n_flow);
  return af_launch_status();
}

extern "C" int arflow_out_tail_fwd(const float* in, long in_bstride, float* out1, float* out0, int B, int C, int h, int w,
                                   int n_flow, int n_diag, float diag_bias, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(out0);
  const int rc = out_up_check(in, in_bstride, out1, (long)C * 4 * h * w, B, C, h, w, n_flow, n_diag, 1, 4);
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
  const int rc = out_up_check(in, in_bstride, out, out_bstride, B, C, h, w, n_flow, n_diag, 1, factor * factor);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(h <= 2048 && w <= 2048, ARFLOW_ESHAPE);
  const long n = (long)B * C * factor * factor * h * w;
  if (((long)factor * w) % 4 == 0 && af_vec4_ok(out, out_bstride, B)) {
    hipLaunchKernelGGL(prob_up_fwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                       in_bstride, out, out_bstride, B, C, h, w, factor, n_flow, n_diag, diag_bias);
  } else {
    hipLaunchKernelGGL(prob_up_fwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                       in_bstride, out, out_bstride, B, C, h, w, factor, n_flow, n_diag, diag_bias);
  }
  return af_launch_status();
}

extern "C" int arflow_prob_up_bwd(const float* gfine, long gfine_bstride, float* gcoarse, long gcoarse_bstride, int B, int C,
                                  int h, int w, int factor, int n_flow, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  const int rc = out_up_check(gfine, gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, n_flow, 0, factor * factor, 1);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(h <= 2048 && w <= 2048, ARFLOW_ESHAPE);
  const long n = (long)B * C * h * w;
  hipLaunchKernelGGL(prob_up_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gfine,
                     gfine_bstride, gcoarse, gcoarse_bstride, B, C, h, w, factor, n_flow);
  return af_launch_status();
}
