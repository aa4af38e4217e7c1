// The SSIM closed form (losses/loss_blocks.py:65-84) of every kernel that computes it: the photometric kernels
// (ssim.hip), the fused warp + mask + L1/SSIM pass (photo_warp.hip) and the any-window kernels (generic.hip).  One
// definition each, so that they agree bit for bit:
//   SSIM_C1 / SSIM_C2, Win, ssim_terms      the constants, a window's five statistics, the four factors of SSIM
//   WinAcc, window_stats<PITCH>             the 3x3 window: nine (x, y) in row-major order, div9 finish
//   div9, fdiv_pos, frcp_pos                the divisions of the tiled kernels
//   ssim_dist, ssim_dist_grad               clamped distance of a window; its gradient coefficients A + B x + C y
//   Coef, rec_grad                          a pixel's coefficient sums and d / d rec (L1 sign included)
//   photo4::                                the 16 x 64 tiling, 4 pixels per lane, templated on the LDS pitch: read6 / read8 /
//                                           stats6, the lane's four forward windows (fwd_windows), the backward's
//                                           coefficient pass (coef_pass) and 3x3 coefficient gather (gather4)
#pragma once
#include "common.hpp"

namespace {

constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Win {
  float mx, my, sx, sy, sxy;
};

// SSIM = n1 n2 / (d1 d2)
struct SsimTerms {
  float n1, n2, d1, d2;
};
__device__ __forceinline__ SsimTerms ssim_terms(const Win& w) {
  return {2.f * w.mx * w.my + SSIM_C1, 2.f * w.sxy + SSIM_C2, w.mx * w.mx + w.my * w.my + SSIM_C1, w.sx + w.sy + SSIM_C2};
}

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

// Running sums of a 3x3 window.  The reference pools the already-rounded products x*x, y*y, x*y (AvgPool2d of a product
// tensor, loss_blocks.py:76-78): round each product, add the nine pixels in row-major order, divide by 9.
// sigma = E[x^2]-mu^2 cancels catastrophically, so the operation order is kept.
struct WinAcc {
  float x = 0.f, y = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
  __device__ __forceinline__ void add(float a, float b) {
    x += a;
    y += b;
    xx += a * a;
    yy += b * b;
    xy += a * b;
  }
  __device__ __forceinline__ Win finish() const {
    Win w;
    w.mx = div9(x);
    w.my = div9(y);
    w.sx = div9(xx) - w.mx * w.mx;
    w.sy = div9(yy) - w.my * w.my;
    w.sxy = div9(xy) - w.mx * w.my;
    return w;
  }
};
// window anchored at (r, c) of two LDS tiles
template <int PITCH>
__device__ __forceinline__ Win window_stats(const float (*tx)[PITCH], const float (*ty)[PITCH], int r, int c) {
  WinAcc s;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s.add(tx[r + i][c + j], ty[r + i][c + j]);
  return s.finish();
}

// dist = clamp((1 - SSIM) / 2, 0, 1) of one window
__device__ __forceinline__ float ssim_dist(const Win& w) {
  const SsimTerms t = ssim_terms(w);
  const float n = t.n1 * t.n2, d = t.d1 * t.d2;
  return fminf(fmaxf((1.f - fdiv_pos(n, d)) / 2.f, 0.f), 1.f);
}
// d dist_w / d x_r = A + B x_r + C y_r for every pixel r of the window (0 where the clamp is active), times the
// upstream coefficient up() (the 2/9 of the window means is folded in).  up is a callable: it is evaluated only where
// the clamp passes the gradient, so a load behind it is not issued for the other windows.
template <class Up>
__device__ __forceinline__ void ssim_dist_grad(const Win& w, Up&& up, float& A, float& Bc, float& Cc) {
  A = Bc = Cc = 0.f;
  const SsimTerms t = ssim_terms(w);
  const float n = t.n1 * t.n2, d = t.d1 * t.d2;
  const float v = (1.f - fdiv_pos(n, d)) / 2.f;
  if (v >= 0.f && v <= 1.f) {  // torch.clamp passes the gradient on the closed interval
    const float k = -0.5f * up() * (2.f / 9.f);
    const float id = frcp_pos(d), nd2 = n * id * id;
    Cc = k * t.n1 * id;                                                             // * y_r
    Bc = -k * nd2 * t.d1;                                                           // * x_r
    A = k * ((w.my * t.n2 - t.n1 * w.my) * id - nd2 * (w.mx * t.d2 - t.d1 * w.mx));  // constant
  }
}

// sums of A, B, C over the (up to) nine windows that hold a pixel
struct Coef {
  float a = 0.f, b = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float A, float Bc, float Cc) {
    a += A;
    b += Bc;
    c += Cc;
  }
};
// d / d rec of c_l1 |im - rec| m + sum_w up_w dist_w at one pixel; x = rec m, y = im m
__device__ __forceinline__ float rec_grad(float m, float c_l1, float rec, float im, const Coef& s, float x, float y) {
  const float diff = rec - im;
  const float sg = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
  return m * (c_l1 * sg + s.a + s.b * x + s.c * y);
}

// ------------------------------------------------------------------------------------------------
// 16 x 64 pixel tile, 256 threads, a lane owns 4 consecutive pixels (xg = lane & 15, ly = lane >> 4) and reads each
// window row as ds_read_b128 + ds_read_b64: 6 values serve its 4 windows.  P: floats per LDS row.
// ------------------------------------------------------------------------------------------------
namespace photo4 {
constexpr int TXW = 64, TYH = 16, NT = 256;
static inline long tiles(long nimg, int H, int W) { return (long)af_cdiv(W, TXW) * af_cdiv(H, TYH) * nimg; }

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
// three rows of six, starting at (r, 4 g) of the tiles X, Y
template <int P>
__device__ __forceinline__ void read_strips(const float* X, const float* Y, int r, int g, float (&a)[3][6], float (&b)[3][6]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    read6(X + (r + i) * P + 4 * g, a[i]);
    read6(Y + (r + i) * P + 4 * g, b[i]);
  }
}
// statistics of the 3x3 window whose left column is `e` of the 6-wide strips
__device__ __forceinline__ Win stats6(const float (&a)[3][6], const float (&b)[3][6], int e) {
  WinAcc s;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s.add(a[i][e + j], b[i][e + j]);
  return s.finish();
}

// Forward: f(e, dist) for the lane's windows anchored at tile (ly, 4 xg + e) = image column x0 + e, e = 0..3, that exist
template <int P, class F>
__device__ __forceinline__ void fwd_windows(const float* X, const float* Y, int ly, int xg, int x0, int W, F&& f) {
  float a[3][6], b[3][6];
  read_strips<P>(X, Y, ly, xg, a, b);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (x0 + e < W - 2) f(e, ssim_dist(stats6(a, b, e)));
}

// Backward tile coordinates: row r <-> image row ty0 - 2 + r (20 rows), column q <-> image column tx0 - 4 + q (72).
// Coefficient pass: A, B, C of the windows anchored at rows 0..17, columns 0..67 (18 x 17 groups of 4 anchors; 0 for a
// window that does not exist) into WA / WB / WC.  up(wy, wx): upstream coefficient of the window anchored at image (wy, wx).
template <int P, class Up>
__device__ __forceinline__ void coef_pass(const float* X, const float* Y, float* WA, float* WB, float* WC, int ty0, int tx0,
                                          int H, int W, Up&& up) {
  constexpr int NG = TXW / 4 + 1, NTASK = (TYH + 2) * NG;
  for (int t = threadIdx.x; t < NTASK; t += NT) {
    const int r = t / NG, g = t - r * NG;
    float a[3][6], b[3][6];
    read_strips<P>(X, Y, r, g, a, b);
    const int wy = ty0 - 2 + r;
    const bool row = wy >= 0 && wy < H - 2;
    float A[4], Bc[4], Cc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int wx = tx0 - 4 + 4 * g + e;
      A[e] = Bc[e] = Cc[e] = 0.f;
      if (row && wx >= 0 && wx < W - 2)
        ssim_dist_grad(stats6(a, b, e), [&] { return up(wy, wx); }, A[e], Bc[e], Cc[e]);
    }
    *reinterpret_cast<float4*>(WA + r * P + 4 * g) = make_float4(A[0], A[1], A[2], A[3]);
    *reinterpret_cast<float4*>(WB + r * P + 4 * g) = make_float4(Bc[0], Bc[1], Bc[2], Bc[3]);
    *reinterpret_cast<float4*>(WC + r * P + 4 * g) = make_float4(Cc[0], Cc[1], Cc[2], Cc[3]);
  }
}
// Gather: pixel (y, x0 + e) = tile (ly + 2, 4 xg + 4 + e); the window anchored at (y - i, x - j) sits at tile
// (ly + 2 - i, 4 xg + 4 + e - j).  f(e, coefficient sums, x, y) for the lane's four pixels.
template <int P, class F>
__device__ __forceinline__ void gather4(const float* X, const float* Y, const float* WA, const float* WB, const float* WC,
                                        int ly, int xg, F&& f) {
  float ca[3][8], cb[3][8], cc[3][8], xc[8], yc[8];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    read8(WA + (ly + i) * P + 4 * xg, ca[i]);
    read8(WB + (ly + i) * P + 4 * xg, cb[i]);
    read8(WC + (ly + i) * P + 4 * xg, cc[i]);
  }
  read8(X + (ly + 2) * P + 4 * xg, xc);
  read8(Y + (ly + 2) * P + 4 * xg, yc);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    Coef s;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) s.add(ca[2 - i][4 + e - j], cb[2 - i][4 + e - j], cc[2 - i][4 + e - j]);
    f(e, s, xc[4 + e], yc[4 + e]);
  }
}
}  // namespace photo4

}  // namespace
