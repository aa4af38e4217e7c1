// The 16 x 64 pixel tile of the 4-pixels-per-lane census kernels (photo.hip, census_warp.hip): grey (x255) tiles
// with a MAXR halo in LDS at a conflict-free pitch, window rows read as three ds_read_b128.
#pragma once
#include "census_dev.hpp"

namespace {
namespace census4 {
constexpr int TXW = 64, TYH = 16, NT = 256, PITCH = 128, MAXR = 3;
constexpr int ROWS = TYH + 2 * MAXR;  // 22 tile rows (R = 3); smaller radii use the top-left part
typedef float f32x4 __attribute__((ext_vector_type(4)));
static inline unsigned grid(int B, int H, int W) { return af_grid_for_tiles((long)af_cdiv(W, TXW) * af_cdiv(H, TYH) * B); }

// grey tile covering image rows [ty0-R, ty0+TYH+R) and columns [tx0-4, tx0+TXW+4), zero outside
template <int R>
__device__ __forceinline__ void load_gray(float* __restrict__ tile, const float* __restrict__ im, int H, int W,
                                          int ty0, int tx0) {
  constexpr int NR = TYH + 2 * R, NQ = (TXW + 8) / 4;  // 18 float4 per row
  const long cs = (long)H * W;
  for (int i = threadIdx.x; i < NR * NQ; i += NT) {
    const int r = i / NQ, q = i - r * NQ;
    const int gy = ty0 - R + r, gx = tx0 - 4 + 4 * q;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const float* p = im + (long)gy * W + gx;
      const float4 a = *reinterpret_cast<const float4*>(p);
      const float4 b = *reinterpret_cast<const float4*>(p + cs);
      const float4 c = *reinterpret_cast<const float4*>(p + 2 * cs);
      g = gray255(a, b, c);
    }
    *reinterpret_cast<float4*>(tile + r * PITCH + 4 * q) = g;
  }
}

// plain plane tile: NR rows from image row gy0, NQ float4 per row from image column gx0 (a multiple of 4), zero outside
template <int NR, int NQ = (TXW + 8) / 4>
__device__ __forceinline__ void load_plane_rows(float* __restrict__ tile, const float* __restrict__ g, int H, int W, int gy0,
                                                int gx0, int tid) {
  for (int i = tid; i < NR * NQ; i += NT) {
    const int r = i / NQ, q = i - r * NQ;
    const int gy = gy0 + r, gx = gx0 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(g + (long)gy * W + gx);
    *reinterpret_cast<float4*>(tile + r * PITCH + 4 * q) = v;
  }
}
// the rectangle of load_gray from a [H,W] plane
template <int R>
__device__ __forceinline__ void load_plane(float* __restrict__ tile, const float* __restrict__ g, int H, int W, int ty0,
                                           int tx0) {
  load_plane_rows<TYH + 2 * R>(tile, g, H, W, ty0 - R, tx0 - 4, threadIdx.x);
}

__device__ __forceinline__ void read12(const float* row, float (&w)[12]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    f32x4 t = *reinterpret_cast<const f32x4*>(row + 4 * q);
    asm volatile("" : "+v"(t));  // keep it one ds_read_b128
    w[4 * q] = t.x, w[4 * q + 1] = t.y, w[4 * q + 2] = t.z, w[4 * q + 3] = t.w;
  }
}

}  // namespace census4
}  // namespace
