// resize_flow of utils/flow_utils.py:110-118 per output pixel, stated once: ATen's bilinear resize
// (no antialiasing) of a two-channel flow [2][H][W] -> (h, w), channel 0 divided by W / w and channel 1 by H / h.
//   align_corners = 0:  src = max(0, (d + 0.5) (n_in / n_out) - 0.5)
//   align_corners = 1:  src = d (n_in - 1) / (n_out - 1), 0 when n_out == 1
//   i0 = min(floor(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  lambda = src - i0
// The source coordinate is formed in float64 (wave-uniform along one axis, a handful of operations per lane) and lambda is
// rounded to fp32 once, so the weights carry one rounding instead of the three of an fp32 coordinate of magnitude n_in; the
// blend is ATen's fp32 expression l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11) under -ffp-contract=off; the division
// by the scale is one float64 division rounded to fp32 once.  Every entry point of mse.hip calls rf_resize_flow.
#pragma once
#include <hip/hip_runtime.h>

struct RfAxis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ RfAxis rf_axis(int d, int n_in, int n_out, int align) {
  double src;
  if (align) {
    src = n_out > 1 ? (double)d * ((double)(n_in - 1) / (double)(n_out - 1)) : 0.0;
  } else {
    src = ((double)d + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    if (src < 0.0) src = 0.0;
  }
  int i0 = (int)src;  // src >= 0: truncation is floor
  if (i0 > n_in - 1) i0 = n_in - 1;
  RfAxis a;
  a.i0 = i0;
  a.i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  a.l1 = (float)(src - (double)i0);
  a.l0 = 1.0f - a.l1;
  return a;
}

__device__ __forceinline__ float rf_blend(const float* __restrict__ p, int W, const RfAxis& y, const RfAxis& x) {
  const float* r0 = p + (long)y.i0 * W;
  const float* r1 = p + (long)y.i1 * W;
  const float top = x.l0 * r0[x.i0] + x.l1 * r0[x.i1];
  const float bot = x.l0 * r1[x.i0] + x.l1 * r1[x.i1];
  return y.l0 * top + y.l1 * bot;
}

// item: one [2][H][W] flow;  (y, x): the output pixel of the (h, w) grid  ->  the two resized, rescaled flow components
__device__ __forceinline__ void rf_resize_flow(const float* __restrict__ item, int H, int W, int h, int w, int y, int x,
                                               int align, float& g0, float& g1) {
  const RfAxis ay = rf_axis(y, H, h, align), ax = rf_axis(x, W, w, align);
  const float v0 = rf_blend(item, W, ay, ax), v1 = rf_blend(item + (long)H * W, W, ay, ax);
  g0 = (float)((double)v0 / ((double)W / (double)w));
  g1 = (float)((double)v1 / ((double)H / (double)h));
}
