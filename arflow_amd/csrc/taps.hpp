// Bilinear sampling taps shared by the warp kernels (warp.hip) and the fused census + warp kernels (photo.hip):
// the arithmetic of torch's grid_sample as the reference calls it (ATen/native/GridSampler.h:27-83 through
// utils/warp_utils.py:83-90 and utils/uflow_utils.py:53-77), computed once per pixel.
#pragma once
#include "common.hpp"
#include "upsample_dev.hpp"  // up_source / up2_source / up_blend: the bilinear resize, for the kernels that warp and resize

namespace {

struct Taps {
  int x0, y0;           // north-west corner
  float wx0, wx1, wy0, wy1;
  bool vx0, vx1, vy0, vy1;  // corner inside the source
  float dx, dy;         // d coord / d flow (0 where border clamping is active)
};

__device__ __forceinline__ Taps make_taps(float px, float py, float u, float v, int H, int W, int Hs,
                                          int Ws, int pad, bool align, int norm) {
  Taps t;
  float ix = af_sample_coord(px, u, W, Ws, norm, align, &t.dx);
  float iy = af_sample_coord(py, v, H, Hs, norm, align, &t.dy);
  if (pad == ARFLOW_PAD_BORDER) {
    ix = af_clip_border(ix, Ws, &t.dx);
    iy = af_clip_border(iy, Hs, &t.dy);
  }
  const float fx = floorf(ix), fy = floorf(iy);
  t.wx1 = ix - fx;
  t.wx0 = (fx + 1.f) - ix;
  t.wy1 = iy - fy;
  t.wy0 = (fy + 1.f) - iy;
  // comparisons in float first: NaN / huge coordinates fall out as "outside"
  t.vx0 = fx >= 0.f && fx <= (float)(Ws - 1);
  t.vx1 = fx + 1.f >= 0.f && fx + 1.f <= (float)(Ws - 1);
  t.vy0 = fy >= 0.f && fy <= (float)(Hs - 1);
  t.vy1 = fy + 1.f >= 0.f && fy + 1.f <= (float)(Hs - 1);
  t.x0 = (t.vx0 || t.vx1) ? (int)fx : 0;
  t.y0 = (t.vy0 || t.vy1) ? (int)fy : 0;
  return t;
}

// Branch-free channel loop: the four tap addresses are clamped into the source once (always
// dereferenceable) and taps outside the image are selected to zero after the load, so all loads of
// several unrolled channels are in flight together (the per-tap `if` form serialised them).
struct TapPlan {
  int o[4];     // element offsets inside one source plane (clamped)
  float w[4];   // bilinear weights
  bool ok[4];   // tap inside the source
};
__device__ __forceinline__ TapPlan plan_taps(const Taps& t, int Hs, int Ws) {
  TapPlan p;
  const int xa = min(max(t.x0, 0), Ws - 1), xb = min(max(t.x0 + 1, 0), Ws - 1);
  const int ya = min(max(t.y0, 0), Hs - 1), yb = min(max(t.y0 + 1, 0), Hs - 1);
  p.o[0] = ya * Ws + xa, p.o[1] = ya * Ws + xb, p.o[2] = yb * Ws + xa, p.o[3] = yb * Ws + xb;
  p.w[0] = t.wx0 * t.wy0, p.w[1] = t.wx1 * t.wy0, p.w[2] = t.wx0 * t.wy1, p.w[3] = t.wx1 * t.wy1;
  p.ok[0] = t.vx0 && t.vy0, p.ok[1] = t.vx1 && t.vy0, p.ok[2] = t.vx0 && t.vy1, p.ok[3] = t.vx1 && t.vy1;
  return p;
}

// The tap arithmetic, stated ONCE: tests compare fused paths against unfused ones bit for bit, so every kernel that
// samples calls these (a[k] = the value loaded at p.o[k]; the loads and their scheduling stay with the caller).
// Bilinear sample, accumulated north-west, north-east, south-west, south-east; a tap outside the source adds nothing.
__device__ __forceinline__ float tap_blend(const TapPlan& p, const float (&a)[4]) {
  float r = p.ok[0] ? a[0] * p.w[0] : 0.f;
  r = p.ok[1] ? fmaf(a[1], p.w[1], r) : r;
  r = p.ok[2] ? fmaf(a[2], p.w[2], r) : r;
  r = p.ok[3] ? fmaf(a[3], p.w[3], r) : r;
  return r;
}
// The taps as the gradient kernels read them: zero outside the source.
__device__ __forceinline__ void tap_select(const TapPlan& p, const float (&a)[4], float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = p.ok[k] ? a[k] : 0.f;
}
// ... read from plane (or LDS window) s at offsets o: only the taps inside the source are read.  The staged flow-gradient
// loop uses this form: with four unconditional LDS reads per channel ahead of the selects warp_bwd_flow_kernel<2> needs
// 66 VGPRs (7 waves per SIMD) instead of 62 (8).
__device__ __forceinline__ void tap_select(const TapPlan& p, const float* __restrict__ s, const int (&o)[4], float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = p.ok[k] ? s[o[k]] : 0.f;
}
// d sample / d coordinate of tap values v (from tap_select): the corner differences along x blended over y, and along
// y blended over x.  Times t.dx / t.dy this is d sample / d flow.
__device__ __forceinline__ void tap_corner_grad(const Taps& t, const float (&v)[4], float& sx, float& sy) {
  sx = (v[1] - v[0]) * t.wy0 + (v[3] - v[2]) * t.wy1;
  sy = (v[2] - v[0]) * t.wx0 + (v[3] - v[1]) * t.wx1;
}

// The four target cells and weights of a forward splat at position (cx, cy) (splat_kernel, warp.hip, and its fixed-order
// form in det_scatter.hip): variant 0 = compute_range_map, 1 = get_corresponding_map (clamped indices, weight dropped when a
// tap left the image).
struct SplatTaps {
  int xi[4], yi[4];
  float w[4];
  bool ok[4];
};
__device__ __forceinline__ SplatTaps splat_taps(float cx, float cy, int H, int W, int variant) {
  SplatTaps t;
  const float fx = floorf(cx), fy = floorf(cy);
  if ((variant & 1) == 0) {
    const float ox = cx - fx, oy = cy - fy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int di = k >> 1, dj = k & 1;
      const float yi = fy + di, xj = fx + dj;
      t.ok[k] = yi >= 0.f && yi < (float)H && xj >= 0.f && xj < (float)W;
      t.w[k] = (di ? oy : 1.f - oy) * (dj ? ox : 1.f - ox);
      t.yi[k] = t.ok[k] ? (int)yi : 0;
      t.xi[k] = t.ok[k] ? (int)xj : 0;
    }
  } else {
    const float xw = (float)(W - 1), yh = (float)(H - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int di = k >> 1, dj = k & 1;
      const float yr = fy + di, xr = fx + dj;
      const float yc = fminf(fmaxf(yr, 0.f), yh), xc = fminf(fmaxf(xr, 0.f), xw);
      t.ok[k] = yc == yr && xc == xr;
      t.w[k] = (1.f - fabsf(cx - xc)) * (1.f - fabsf(cy - yc));
      t.yi[k] = t.ok[k] ? (int)yc : 0;
      t.xi[k] = t.ok[k] ? (int)xc : 0;
    }
  }
  return t;
}

__device__ __forceinline__ Taps no_taps() {
  Taps t;
  t.vx0 = t.vx1 = t.vy0 = t.vy1 = false;
  t.x0 = t.y0 = 0;
  t.wx0 = t.wx1 = t.wy0 = t.wy1 = t.dx = t.dy = 0.f;
  return t;
}

}  // namespace
