// Device code of the 3x3 SSIM closed form shared by the photometric kernels (ssim.hip) and the fused warp + mask +
// L1/SSIM pass (photo_warp.hip): losses/loss_blocks.py:65-84.  One definition, so the two agree bit for bit.
#pragma once
#include "common.hpp"

namespace {

constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Win {
  float mx, my, sx, sy, sxy;
};

// x / 9 exactly as IEEE division rounds it, in 3 VALU instructions instead of the ~12 of the generic
// sequence: q = x*c; r = fma(-9, q, x); q = fma(r, c, q) with c = RN(1/9).  Bit-identical to x / 9.0f for
// every finite float (all 2^32 patterns compared on the GPU, tools/ubench/div9_check.hip; only +-inf and one
// value next to overflow differ).  The SSIM kernels are VALU-bound and did six divisions per window.
__device__ __forceinline__ float div9(float x) {
  const float c = 1.0f / 9.0f;
  float q = x * c;
  const float r = fmaf(-9.0f, q, x);
  return fmaf(r, c, q);
}
// n / d and 1 / d for d > 0 (the SSIM denominators are >= C1*C2 > 0): hardware reciprocal + one Newton
// step, within 1 ulp of the IEEE quotient (enters (1 - n/d)/2 with absolute error <= 6e-8).
__device__ __forceinline__ float fdiv_pos(float n, float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  const float q = n * r;
  return fmaf(fmaf(-d, q, n), r, q);
}
__device__ __forceinline__ float frcp_pos(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.0f), r, r);
}

// dist = clamp((1 - SSIM) / 2, 0, 1) of one window
__device__ __forceinline__ float ssim_dist(const Win& w) {
  const float n = (2.f * w.mx * w.my + SSIM_C1) * (2.f * w.sxy + SSIM_C2);
  const float d = (w.mx * w.mx + w.my * w.my + SSIM_C1) * (w.sx + w.sy + SSIM_C2);
  return fminf(fmaxf((1.f - fdiv_pos(n, d)) / 2.f, 0.f), 1.f);
}
// d dist_w / d x_r = A + B x_r + C y_r for every pixel r of the window (0 where the clamp is active), times the
// upstream coefficient `up` (the 2/9 of the window means is folded in)
__device__ __forceinline__ void ssim_dist_grad(const Win& w, float up, float& A, float& Bc, float& Cc) {
  A = Bc = Cc = 0.f;
  const float n1 = 2.f * w.mx * w.my + SSIM_C1, n2 = 2.f * w.sxy + SSIM_C2;
  const float d1 = w.mx * w.mx + w.my * w.my + SSIM_C1, d2 = w.sx + w.sy + SSIM_C2;
  const float n = n1 * n2, d = d1 * d2;
  const float v = (1.f - fdiv_pos(n, d)) / 2.f;
  if (v >= 0.f && v <= 1.f) {  // torch.clamp passes the gradient on the closed interval
    const float k = -0.5f * up * (2.f / 9.f);
    const float id = frcp_pos(d), nd2 = n * id * id;
    Cc = k * n1 * id;                                                     // * y_r
    Bc = -k * nd2 * d1;                                                   // * x_r
    A = k * ((w.my * n2 - n1 * w.my) * id - nd2 * (w.mx * d2 - d1 * w.mx));  // constant
  }
}

namespace photo4 {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void read6(const float* row, float (&v)[6]) {
  f32x4 t = *reinterpret_cast<const f32x4*>(row);
  f32x2 u = *reinterpret_cast<const f32x2*>(row + 4);
  asm volatile("" : "+v"(t), "+v"(u));
  v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w, v[4] = u.x, v[5] = u.y;
}
__device__ __forceinline__ void read8(const float* row, float (&v)[8]) {
  f32x4 t = *reinterpret_cast<const f32x4*>(row);
  f32x4 u = *reinterpret_cast<const f32x4*>(row + 4);
  asm volatile("" : "+v"(t), "+v"(u));
  v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w, v[4] = u.x, v[5] = u.y, v[6] = u.z, v[7] = u.w;
}
// statistics of the 3x3 window whose left column is `e` of the 6-wide strips (same order as window_stats)
__device__ __forceinline__ Win stats6(const float (&a)[3][6], const float (&b)[3][6], int e) {
  float sxv = 0.f, syv = 0.f, sxx = 0.f, syy = 0.f, sxyv = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      // the reference pools the already-rounded products x*x, y*y, x*y (AvgPool2d of a product
      // tensor, loss_blocks.py:76-78): round each product, add in row-major order, divide by 9.
      const float x = a[i][e + j], y = b[i][e + j];
      sxv += x;
      syv += y;
      sxx += x * x;
      syy += y * y;
      sxyv += x * y;
    }
  Win w;
  w.mx = div9(sxv);
  w.my = div9(syv);
  w.sx = div9(sxx) - w.mx * w.mx;
  w.sy = div9(syy) - w.my * w.my;
  w.sxy = div9(sxyv) - w.mx * w.my;
  return w;
}
}  // namespace photo4

}  // namespace
