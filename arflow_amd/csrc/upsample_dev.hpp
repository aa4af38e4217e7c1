// The bilinear resize, stated once: source index and weights, the blend, the channel rule of the
// output upsamples, the forward pixel group and the two forms of the gather adjoint.  upsample.hip builds every resize
// kernel from these; warp.hip, level_small.hip, flow_eval.hip and uncert.hip use up_source / up2_source / up_blend
// through taps.hpp.
#pragma once
#include "common.hpp"

namespace {

// Source rows / weights of output index d of the bilinear resize n_in -> n_out: ATen/native/UpSample.h
// area_pixel_compute_source_index + the index / lambda arithmetic of upsample_bilinear2d.  rs is the half-pixel scale of
// the align_corners=False map: 1 / scale_factor where the caller of F.interpolate gave one (upsample.hip, the level's x2),
// (float)n_in / n_out where it gave a size (flow_eval.hip; cv2.INTER_LINEAR is the same map).  Both taps are clamped.
__device__ __forceinline__ void up_source(int d, int n_in, int n_out, float rs, bool align, int& i0, int& i1, float& l0,
                                          float& l1) {
  float src;
  if (align) {
    const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
    src = scale * (float)d;
  } else {
    src = rs * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
  }
  i0 = min((int)src, n_in - 1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}
// ... the x2 case n_out = 2 n_in of the fused level (scale_factor = 2 given: scale = 1 / 2)
__device__ __forceinline__ void up2_source(int d, int n_in, int n_out, bool align, int& i0, int& i1, float& l0,
                                           float& l1) {
  up_source(d, n_in, n_out, 0.5f, align, i0, i1, l0, l1);
}
// ... and the blend of the four taps in ATen's order (rows of the x blend, then y); no contraction (-ffp-contract=off)
__device__ __forceinline__ float up_blend(float wx0, float wx1, float wy0, float wy1, float a00, float a01, float a10,
                                          float a11) {
  return wy0 * (wx0 * a00 + wx1 * a01) + wy1 * (wx0 * a10 + wx1 * a11);
}

// Gather adjoints of the resize: one thread per coarse cell (i, j).  The fine rows that read coarse row i are those whose
// source index i0 is i or i - 1, i.e. src in [i - 1, i + 1): a run of consecutive rows found from the inverse of the source
// map and widened by two on either side -- the weights themselves come from up_source, so a row outside the true run simply weighs 0 and the margin
// only has to be generous, not exact.  Rows ascending, columns ascending inside a row: a fixed order.
__device__ __forceinline__ void fine_run(int i, int n_in, int n_out, int factor, bool align, int& lo, int& hi) {
  if (align) {
    const float inv = n_in > 1 ? (float)(n_out - 1) / (float)(n_in - 1) : (float)n_out;  // fine rows per coarse row
    lo = (int)floorf((float)(i - 1) * inv) - 2;
    hi = (int)ceilf((float)(i + 1) * inv) + 2;
  } else {
    lo = factor * (i - 1) - 2;
    hi = factor * (i + 2) + 2;
  }
  lo = max(lo, 0), hi = min(hi, n_out - 1);
}

// The weight of coarse index i in fine index d: at the image border both clamped taps of d can be i, then they add.
__device__ __forceinline__ float up_weight(int d, int i, int n_in, int n_out, float rs, bool align) {
  int a0, a1;
  float l0, l1;
  up_source(d, n_in, n_out, rs, align, a0, a1, l0, l1);
  return (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
}

// Channel rule of the output upsamples: out[b,c] = s_c * resize(in[b,c] + b_c), s_c = factor for the n_flow flow channels
// else 1, b_c = diag_bias for the n_diag channels after them else 0.
__device__ __forceinline__ float up_chan_scale(int c, int n_flow, int factor) { return c < n_flow ? (float)factor : 1.f; }
__device__ __forceinline__ void up_chan_rule(int c, int n_flow, int n_diag, float diag_bias, int factor, float& s, float& b) {
  s = up_chan_scale(c, n_flow, factor);
  b = (c >= n_flow && c < n_flow + n_diag) ? diag_bias : 0.f;
}

// Forward: V fine pixels x0 .. x0 + V - 1 of fine row y of one plane (src: h x w, dst row: W wide).  The row's two source
// rows and y weights first, then V column blends, then one float4 store (V = 4) or V scalar ones.  BIAS: the bias is added
// to every tap on load, also where it is 0 (a -0.0 tap then reads +0.0; without BIAS it stays -0.0); the power-of-two
// scale follows the blend: the reference's order, and exact.
template <int V, bool BIAS>
__device__ __forceinline__ void up_fwd_group(const float* __restrict__ src, float* __restrict__ dst_row, int y, int x0, int h,
                                             int w, int H, int W, float rs, bool align, float sc, float bias) {
  int ya, yb;
  float wy0, wy1;
  up_source(y, h, H, rs, align, ya, yb, wy0, wy1);
  const float* ra = src + (long)ya * w;
  const float* rb = src + (long)yb * w;
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int xa, xb;
    float wx0, wx1;
    up_source(x0 + k, w, W, rs, align, xa, xb, wx0, wx1);
    if constexpr (BIAS) {
      r[k] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa] + bias, ra[xb] + bias, rb[xa] + bias, rb[xb] + bias);
    } else {
      r[k] = sc * up_blend(wx0, wx1, wy0, wy1, ra[xa], ra[xb], rb[xa], rb[xb]);
    }
  }
  float* o = dst_row + x0;
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = r[k];
  }
}

// Adjoint of one coarse cell (i, j) of a x2 resize, static form: the N x N fine pixels from (y0, x0), the column weights
// once per cell, the loops unrolled, rows ascending, columns ascending inside a row; a pixel outside the image is skipped,
// not read.  N = 4 from (2i - 1, 2j - 1) is exact for align_corners=False.  g: the cell's fine plane (H x W).  Returns the
// unscaled sum.  (up2_bwd_kernel, upsample.hip, is the N = 6 case from 2i - 2 that reads such a pixel at the clamped index
// with weight 0; it is the hot path's kernel and keeps its own body)
template <int N>
__device__ __forceinline__ float up_gather_static(const float* __restrict__ g, int i, int j, int y0, int x0, int h, int w, int H,
                                                  int W, bool align) {
  float wx[N];
  bool vx[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    vx[k] = x0 + k >= 0 && x0 + k < W;
    wx[k] = up_weight(vx[k] ? x0 + k : 0, j, w, W, 0.5f, align);
  }
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    const int y = y0 + r;
    if (y < 0 || y >= H) continue;
    const float wy = up_weight(y, i, h, H, 0.5f, align);
    const float* gr = g + (long)y * W + x0;
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (vx[k]) row = fmaf(wx[k], gr[k], row);
    acc = fmaf(wy, row, acc);
  }
  return acc;
}

// ... run form, any factor: fine_run's rows and columns (generous: a fine pixel that does not read the cell weighs 0).
// The column weights are the same for every row: the first UP_RUN_COLS of the run are computed once and kept in
// registers (for factors 2 and 4 with align_corners=True the run is at most 2 * 5 + 5 = 15 columns wide once w >= 4, and
// at most W <= 12 below that); columns beyond them, where a run is wider (factor 4 without align_corners: 17), are
// weighed where they are used.  Same weights, same order of additions.
constexpr int UP_RUN_COLS = 16;
__device__ __forceinline__ float up_gather_run(const float* __restrict__ g, int i, int j, int h, int w, int H, int W, int factor,
                                               float rs, bool align) {
  int ylo, yhi, xlo, xhi;
  fine_run(i, h, H, factor, align, ylo, yhi);
  fine_run(j, w, W, factor, align, xlo, xhi);
  float wx[UP_RUN_COLS];
#pragma unroll
  for (int k = 0; k < UP_RUN_COLS; ++k) wx[k] = up_weight(min(xlo + k, W - 1), j, w, W, rs, align);
  float acc = 0.f;
  for (int y = ylo; y <= yhi; ++y) {
    const float wy = up_weight(y, i, h, H, rs, align);
    const float* gr = g + (long)y * W;
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < UP_RUN_COLS; ++k)
      if (xlo + k <= xhi) row = fmaf(wx[k], gr[xlo + k], row);
    for (int x = xlo + UP_RUN_COLS; x <= xhi; ++x) row = fmaf(up_weight(x, j, w, W, rs, align), gr[x], row);
    acc = fmaf(wy, row, acc);
  }
  return acc;
}

}  // namespace
