// Flow rendering and original-size restore: what a user does with a network output.
//   arflow_restore_out    inference.py:98-107: flow (and entropy) at test size -> NHWC at the original size, with the
//                         per-sample maxima the renderers normalise by, in one pass
//   arflow_flow_stats     the same maxima of a flow already at its final size
//   arflow_flow_render    np_flow2rgb (utils/flow_utils.py:84-96) / flow_to_image (:67-81) per pixel
//   arflow_scalar_stats / arflow_scalar_render   the entropy picture of trainer/uflow_elbo_trainer.py:259-262
// The resize is rf_axis / rf_blend of resize_dev.hpp (align = 0).  Maxima and minima are integer atomics on the float bits
// (a maximum does not depend on the order), in front of which a tiny kernel stores the identities.  Every index is clamped
// before an address is formed; a lane beyond the image computes on the clamped pixel and stores nothing.
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "resize_dev.hpp"

#define RN_NT 256
#define RN_PX 4  // pixels per lane of the flat (render / stats) kernels

// ---- order-free float maxima / minima ------------------------------------------------------------------------------
// Non-negative floats order as their bits read as signed integers, negative ones in reverse as unsigned ones, so one
// integer atomic per value keeps the float maximum (minimum) whatever float the slot already holds.  No NaN handling.
__device__ __forceinline__ void rn_atomic_max(float* p, float v) {
  const unsigned bits = __float_as_uint(v);
  if (!(bits >> 31)) atomicMax(reinterpret_cast<int*>(p), (int)bits);
  else atomicMin(reinterpret_cast<unsigned*>(p), bits);
}
__device__ __forceinline__ void rn_atomic_min(float* p, float v) {
  const unsigned bits = __float_as_uint(v);
  if (!(bits >> 31)) atomicMin(reinterpret_cast<int*>(p), (int)bits);
  else atomicMax(reinterpret_cast<unsigned*>(p), bits);
}
__device__ __forceinline__ float rn_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, AF_WAVE));
  return v;
}
// (a, b) -> (max a, max b) over the RN_NT threads of the workgroup, valid in thread 0.  All threads must call.
__device__ __forceinline__ void rn_block_max2(float& a, float& b) {
  __shared__ float part[2][RN_NT / AF_WAVE];
  const int t = threadIdx.x + blockDim.x * threadIdx.y, lane = t & 63, wave = t >> 6;
  a = rn_wave_max(a), b = rn_wave_max(b);
  if (lane == 0) part[0][wave] = a, part[1][wave] = b;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < RN_NT / AF_WAVE; ++w) a = fmaxf(a, part[0][w]), b = fmaxf(b, part[1][w]);
  }
}

// identities: pairs (lo, hi) stored into n rows of 2 floats
__global__ void rn_init_kernel(float* __restrict__ rows, int n, float lo, float hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) *reinterpret_cast<float2*>(rows + 2 * (long)i) = make_float2(lo, hi);
}
static void rn_init(float* rows, int n, float lo, float hi, hipStream_t s) {
  hipLaunchKernelGGL(rn_init_kernel, dim3(af_cdiv(n, RN_NT)), dim3(RN_NT), 0, s, rows, n, lo, hi);
}

// ---- restore ----------------------------------------------------------------------------------------------------------
struct RsArgs {
  const float *flow, *ent;
  long flow_bs, ent_bs;
  float *out_flow, *out_ent, *stats;
  int h, w, H, W;
  double sx, sy, shx, shy;  // W / w, H / h, 2 log W - 2 log w, 2 log H - 2 log h
};

// Workgroup (64, 4): 4 rows of 128 output pixels, two adjacent pixels per lane = one float4 of NHWC.  VEC: W even and the
// outputs 16-byte aligned (host-checked), so x0 < W implies x0 + 1 < W and the address is aligned; else float-by-float.
template <bool VEC>
__global__ __launch_bounds__(RN_NT) void restore_out_kernel(RsArgs a) {
  const int b = blockIdx.z;
  const int y = blockIdx.y * 4 + threadIdx.y, x0 = (blockIdx.x * 64 + threadIdx.x) * 2;
  const bool row_ok = y < a.H;
  const RfAxis ay = rf_axis(row_ok ? y : a.H - 1, a.h, a.H, 0);
  const long hw = (long)a.h * a.w;
  const float* fl = a.flow + (long)b * a.flow_bs;
  const float* en = a.ent ? a.ent + (long)b * a.ent_bs : nullptr;
  float f[4], e[4] = {0.f, 0.f, 0.f, 0.f};
  float amax = 0.f, smax = -INFINITY;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bool ok = row_ok && x0 + j < a.W;
    const RfAxis ax = rf_axis(x0 + j < a.W ? x0 + j : a.W - 1, a.w, a.W, 0);
    f[2 * j] = (float)((double)rf_blend(fl, a.w, ay, ax) * a.sx);
    f[2 * j + 1] = (float)((double)rf_blend(fl + hw, a.w, ay, ax) * a.sy);
    if (ok) {
      amax = fmaxf(amax, fmaxf(fabsf(f[2 * j]), fabsf(f[2 * j + 1])));
      smax = fmaxf(smax, fmaxf(f[2 * j], f[2 * j + 1]));
    }
    if (en) {
      e[2 * j] = (float)((double)rf_blend(en, a.w, ay, ax) + a.shx);
      e[2 * j + 1] = (float)((double)rf_blend(en + hw, a.w, ay, ax) + a.shy);
    }
  }
  if (row_ok && x0 < a.W) {
    const long o = (((long)b * a.H + y) * a.W + x0) * 2;
    if (VEC) {
      *reinterpret_cast<float4*>(a.out_flow + o) = make_float4(f[0], f[1], f[2], f[3]);
      if (en) *reinterpret_cast<float4*>(a.out_ent + o) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
      const int n = x0 + 1 < a.W ? 4 : 2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) a.out_flow[o + k] = f[k];
        if (k < n && en) a.out_ent[o + k] = e[k];
      }
    }
  }
  if (a.stats) {  // wave-uniform
    rn_block_max2(amax, smax);
    if (threadIdx.x == 0 && threadIdx.y == 0) {
      atomicMax(reinterpret_cast<unsigned*>(a.stats + 2 * b), __float_as_uint(amax));
      rn_atomic_max(a.stats + 2 * b + 1, smax);
    }
  }
}

// ---- flat kernels: RN_PX consecutive pixels of one sample per lane ------------------------------------------------------
// VEC: H W a multiple of 4 and every pointer and stride on a 16-byte boundary (host-checked), so q < HW implies q + 3 < HW.
// Otherwise every element is read at a clamped index and stored under its own guard.
template <bool VEC>
__device__ __forceinline__ void rn_ld_plane4(const float* __restrict__ p, long q, long HW, float (&v)[4]) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p + q);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[q + j < HW ? q + j : HW - 1];
  }
}
template <bool VEC>
__device__ __forceinline__ void rn_ld_flow4(const float* __restrict__ fl, int layout, long q, long HW, float (&u)[4],
                                            float (&v)[4]) {
  if (layout == ARFLOW_LAYOUT_NCHW) {
    rn_ld_plane4<VEC>(fl, q, HW, u);
    rn_ld_plane4<VEC>(fl + HW, q, HW, v);
  } else if (VEC) {
    const float4 s = *reinterpret_cast<const float4*>(fl + 2 * q), t = *reinterpret_cast<const float4*>(fl + 2 * q + 4);
    u[0] = s.x, v[0] = s.y, u[1] = s.z, v[1] = s.w, u[2] = t.x, v[2] = t.y, u[3] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = q + j < HW ? q + j : HW - 1;
      u[j] = fl[2 * i], v[j] = fl[2 * i + 1];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(RN_NT) void flow_stats_kernel(const float* __restrict__ flow, long flow_bs, int layout,
                                                           float* __restrict__ stats, long HW) {
  const int b = blockIdx.y;
  const float* fl = flow + (long)b * flow_bs;
  float amax = 0.f, smax = -INFINITY;
  for (long q = ((long)blockIdx.x * RN_NT + threadIdx.x) * RN_PX; q < HW; q += (long)gridDim.x * RN_NT * RN_PX) {
    float u[4], v[4];
    rn_ld_flow4<VEC>(fl, layout, q, HW, u, v);  // a clamped element repeats a pixel of the sample: the maxima do not change
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      amax = fmaxf(amax, fmaxf(fabsf(u[j]), fabsf(v[j])));
      smax = fmaxf(smax, fmaxf(u[j], v[j]));
    }
  }
  rn_block_max2(amax, smax);
  if (threadIdx.x == 0) {
    atomicMax(reinterpret_cast<unsigned*>(stats + 2 * b), __float_as_uint(amax));
    rn_atomic_max(stats + 2 * b + 1, smax);
  }
}

__device__ __forceinline__ float rn_clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ unsigned rn_u8(float c) { return (unsigned)(int)(255.f * c); }  // c in [0,1]: truncation

// one pixel -> (r, g, b) in [0,1].  ok: the scale is positive and finite.
__device__ __forceinline__ void rn_colour(int mode, float u, float v, float scale, bool ok, float& r, float& g, float& b) {
  if (mode == ARFLOW_RENDER_RGB) {
    const float nu = ok ? u / scale : 0.f, nv = ok ? v / scale : 0.f;
    r = rn_clip01(1.f + nu);
    g = rn_clip01(1.f - 0.5f * (nu + nv));
    b = rn_clip01(1.f + nv);
    return;
  }
  const float mag = sqrtf(u * u + v * v);
  float h = atan2f(v, u) / 6.2831855f + 1.f;  // in [0.5, 1.5]
  h = h - floorf(h);
  const float sat = ok ? rn_clip01(mag * 8.f / scale) : 0.f;
  const float val = rn_clip01(8.f - sat);
  const float h6 = h * 6.f;
  const int i = (int)h6;
  const float f = h6 - (float)i;
  const float p = val * (1.f - sat), q = val * (1.f - sat * f), t = val * (1.f - sat * (1.f - f));
  const int k = i % 6;
  r = k == 0 || k == 5 ? val : k == 1 ? q : k == 4 ? t : p;
  g = k == 1 || k == 2 ? val : k == 0 ? t : k == 3 ? q : p;
  b = k == 3 || k == 4 ? val : k == 2 ? t : k == 5 ? q : p;
  if (sat == 0.f) r = g = b = val;
}

template <bool VEC>
__global__ __launch_bounds__(RN_NT) void flow_render_kernel(const float* __restrict__ flow, long flow_bs, int layout,
                                                            const float* __restrict__ scale, int scale_stride,
                                                            void* __restrict__ out, int out_kind, int mode, long HW) {
  const int b = blockIdx.y;
  const long q = ((long)blockIdx.x * RN_NT + threadIdx.x) * RN_PX;
  if (q >= HW) return;
  const float s = scale[(long)b * scale_stride];
  const bool ok = s > 0.f && s <= FLT_MAX;
  float u[4], v[4], c[3][4];
  rn_ld_flow4<VEC>(flow + (long)b * flow_bs, layout, q, HW, u, v);
#pragma unroll
  for (int j = 0; j < 4; ++j) rn_colour(mode, u[j], v[j], s, ok, c[0][j], c[1][j], c[2][j]);
  if (out_kind == ARFLOW_RENDER_F32) {
    float* o = reinterpret_cast<float*>(out) + (long)b * 3 * HW + q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (VEC) {
        *reinterpret_cast<float4*>(o + k * HW) = make_float4(c[k][0], c[k][1], c[k][2], c[k][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (q + j < HW) o[k * HW + j] = c[k][j];
      }
    }
    return;
  }
  unsigned char* o = reinterpret_cast<unsigned char*>(out) + ((long)b * HW + q) * 3;
  if (VEC) {  // 12 bytes r g b r | g b r g | b r g b, little-endian; ((b HW + q) 3) is a multiple of 4
    unsigned by[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) by[3 * j + k] = rn_u8(c[k][j]);
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int d = 0; d < 3; ++d) o4[d] = by[4 * d] | by[4 * d + 1] << 8 | by[4 * d + 2] << 16 | by[4 * d + 3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q + j < HW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * j + k] = (unsigned char)rn_u8(c[k][j]);
      }
  }
}

// e = sum_c x_c, channels added in index order
template <bool VEC>
__device__ __forceinline__ void rn_ld_sum4(const float* __restrict__ x, int C, long q, long HW, float (&e)[4]) {
  rn_ld_plane4<VEC>(x, q, HW, e);
  for (int c = 1; c < C; ++c) {
    float t[4];
    rn_ld_plane4<VEC>(x + c * HW, q, HW, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = e[j] + t[j];
  }
}

template <bool VEC>
__global__ __launch_bounds__(RN_NT) void scalar_stats_kernel(const float* __restrict__ x, long x_bs, int C,
                                                             float* __restrict__ minmax, long HW) {
  const float* xb = x + (long)blockIdx.y * x_bs;
  float nmin = -INFINITY, mx = -INFINITY;  // nmin = max(-e): one reduction serves both
  for (long q = ((long)blockIdx.x * RN_NT + threadIdx.x) * RN_PX; q < HW; q += (long)gridDim.x * RN_NT * RN_PX) {
    float e[4];
    rn_ld_sum4<VEC>(xb, C, q, HW, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) nmin = fmaxf(nmin, -e[j]), mx = fmaxf(mx, e[j]);
  }
  rn_block_max2(nmin, mx);
  if (threadIdx.x == 0) {
    rn_atomic_min(minmax, -nmin);
    rn_atomic_max(minmax + 1, mx);
  }
}

template <bool VEC>
__global__ __launch_bounds__(RN_NT) void scalar_render_kernel(const float* __restrict__ x, long x_bs, int C,
                                                              const float* __restrict__ minmax, void* __restrict__ out,
                                                              int out_kind, long HW) {
  const int b = blockIdx.y;
  const long q = ((long)blockIdx.x * RN_NT + threadIdx.x) * RN_PX;
  if (q >= HW) return;
  const float mn = minmax[0], range = minmax[1] - minmax[0];
  float e[4];
  rn_ld_sum4<VEC>(x + (long)b * x_bs, C, q, HW, e);
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = range > 0.f ? (e[j] - mn) / range : 0.f;
  if (out_kind == ARFLOW_RENDER_F32) {
    float* o = reinterpret_cast<float*>(out) + (long)b * HW + q;
    if (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q + j < HW) o[j] = e[j];
    }
    return;
  }
  unsigned char* o = reinterpret_cast<unsigned char*>(out) + (long)b * HW + q;
  if (VEC) {
    *reinterpret_cast<unsigned*>(o) = rn_u8(e[0]) | rn_u8(e[1]) << 8 | rn_u8(e[2]) << 16 | rn_u8(e[3]) << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q + j < HW) o[j] = (unsigned char)rn_u8(e[j]);
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------
#define RN_MAX_DIM 65535

static int rn_check_image(int B, int H, int W) {
  AF_REQUIRE(B >= 1 && B <= RN_MAX_DIM && H >= 1 && W >= 1 && H <= RN_MAX_DIM && W <= RN_MAX_DIM, ARFLOW_ESHAPE);
  return ARFLOW_OK;
}
static unsigned rn_flat_blocks(long HW) { return (unsigned)af_cdiv(HW, (long)RN_NT * RN_PX); }
// reduction passes: grid-stride from ~2048 workgroups in all
static unsigned rn_stat_blocks(long HW, int B) {
  const long nb = rn_flat_blocks(HW), want = (2048 + B - 1) / B;
  return (unsigned)(nb < want ? nb : want);
}

extern "C" int arflow_restore_out(const float* flow, long flow_bstride, const float* ent, long ent_bstride, float* out_flow,
                                  float* out_ent, float* stats, int B, int h, int w, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(out_flow);
  AF_REQUIRE((ent == nullptr) == (out_ent == nullptr), ARFLOW_ENULL);
  int rc = rn_check_image(B, H, W);
  if (rc != ARFLOW_OK) return rc;
  rc = rn_check_image(B, h, w);
  if (rc != ARFLOW_OK) return rc;
  const long hw = (long)h * w;
  AF_REQUIRE(flow_bstride >= 2 * hw && (!ent || ent_bstride >= 2 * hw), ARFLOW_ESHAPE);
  RsArgs a = {flow, ent, flow_bstride, ent_bstride, out_flow, out_ent, stats, h, w, H, W,
              (double)W / (double)w, (double)H / (double)h, 2.0 * std::log((double)W) - 2.0 * std::log((double)w),
              2.0 * std::log((double)H) - 2.0 * std::log((double)h)};
  const hipStream_t s = (hipStream_t)stream;
  if (stats) {
    rn_init(stats, B, 0.f, -INFINITY, s);
    AF_LAUNCH_CHECK();
  }
  const dim3 grid(af_cdiv(W, 128), af_cdiv(H, 4), B), block(64, 4);
  if (W % 2 == 0 && af_aligned16(out_flow) && af_aligned16(out_ent))
    hipLaunchKernelGGL(restore_out_kernel<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(restore_out_kernel<false>, grid, block, 0, s, a);
  return af_launch_status();
}

static int rn_check_flow(const float* flow, long flow_bstride, int layout, int B, int H, int W) {
  AF_REQUIRE_PTR(flow);
  const int rc = rn_check_image(B, H, W);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(flow_bstride >= 2L * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(layout == ARFLOW_LAYOUT_NCHW || layout == ARFLOW_LAYOUT_NHWC, ARFLOW_EPARAM);
  return ARFLOW_OK;
}

extern "C" int arflow_flow_stats(const float* flow, long flow_bstride, int layout, float* stats, int B, int H, int W,
                                 arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(stats);
  const int rc = rn_check_flow(flow, flow_bstride, layout, B, H, W);
  if (rc != ARFLOW_OK) return rc;
  const long HW = (long)H * W;
  const hipStream_t s = (hipStream_t)stream;
  rn_init(stats, B, 0.f, -INFINITY, s);
  AF_LAUNCH_CHECK();
  const dim3 grid(rn_stat_blocks(HW, B), B);
  if (HW % 4 == 0 && af_vec4_ok(flow, flow_bstride, B))
    hipLaunchKernelGGL(flow_stats_kernel<true>, grid, dim3(RN_NT), 0, s, flow, flow_bstride, layout, stats, HW);
  else
    hipLaunchKernelGGL(flow_stats_kernel<false>, grid, dim3(RN_NT), 0, s, flow, flow_bstride, layout, stats, HW);
  return af_launch_status();
}

extern "C" int arflow_flow_render(const float* flow, long flow_bstride, int layout, const float* scale, int scale_stride,
                                  void* out, int out_kind, int mode, int B, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(scale);
  AF_REQUIRE_PTR(out);
  const int rc = rn_check_flow(flow, flow_bstride, layout, B, H, W);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(scale_stride >= 0, ARFLOW_ESHAPE);
  AF_REQUIRE(out_kind == ARFLOW_RENDER_U8 || out_kind == ARFLOW_RENDER_F32, ARFLOW_EPARAM);
  AF_REQUIRE(mode == ARFLOW_RENDER_RGB || mode == ARFLOW_RENDER_WHEEL, ARFLOW_EPARAM);
  const long HW = (long)H * W;
  const dim3 grid(rn_flat_blocks(HW), B);
  const hipStream_t s = (hipStream_t)stream;
  if (HW % 4 == 0 && af_vec4_ok(flow, flow_bstride, B) && af_aligned16(out))
    hipLaunchKernelGGL(flow_render_kernel<true>, grid, dim3(RN_NT), 0, s, flow, flow_bstride, layout, scale, scale_stride, out,
                       out_kind, mode, HW);
  else
    hipLaunchKernelGGL(flow_render_kernel<false>, grid, dim3(RN_NT), 0, s, flow, flow_bstride, layout, scale, scale_stride, out,
                       out_kind, mode, HW);
  return af_launch_status();
}

static int rn_check_scalar(const float* x, long x_bstride, int C, int B, int H, int W) {
  AF_REQUIRE_PTR(x);
  const int rc = rn_check_image(B, H, W);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(C >= 1 && C <= 16, ARFLOW_EPARAM);
  AF_REQUIRE(x_bstride >= (long)C * H * W, ARFLOW_ESHAPE);
  return ARFLOW_OK;
}

extern "C" int arflow_scalar_stats(const float* x, long x_bstride, int C, float* minmax, int B, int H, int W,
                                   arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(minmax);
  const int rc = rn_check_scalar(x, x_bstride, C, B, H, W);
  if (rc != ARFLOW_OK) return rc;
  const long HW = (long)H * W;
  const hipStream_t s = (hipStream_t)stream;
  rn_init(minmax, 1, INFINITY, -INFINITY, s);
  AF_LAUNCH_CHECK();
  const dim3 grid(rn_stat_blocks(HW, B), B);
  if (HW % 4 == 0 && af_vec4_ok(x, x_bstride, B))
    hipLaunchKernelGGL(scalar_stats_kernel<true>, grid, dim3(RN_NT), 0, s, x, x_bstride, C, minmax, HW);
  else
    hipLaunchKernelGGL(scalar_stats_kernel<false>, grid, dim3(RN_NT), 0, s, x, x_bstride, C, minmax, HW);
  return af_launch_status();
}

extern "C" int arflow_scalar_render(const float* x, long x_bstride, int C, const float* minmax, void* out, int out_kind, int B,
                                    int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(minmax);
  AF_REQUIRE_PTR(out);
  const int rc = rn_check_scalar(x, x_bstride, C, B, H, W);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(out_kind == ARFLOW_RENDER_U8 || out_kind == ARFLOW_RENDER_F32, ARFLOW_EPARAM);
  const long HW = (long)H * W;
  const dim3 grid(rn_flat_blocks(HW), B);
  const hipStream_t s = (hipStream_t)stream;
  if (HW % 4 == 0 && af_vec4_ok(x, x_bstride, B) && af_aligned16(out))
    hipLaunchKernelGGL(scalar_render_kernel<true>, grid, dim3(RN_NT), 0, s, x, x_bstride, C, minmax, out, out_kind, HW);
  else
    hipLaunchKernelGGL(scalar_render_kernel<false>, grid, dim3(RN_NT), 0, s, x, x_bstride, C, minmax, out, out_kind, HW);
  return af_launch_status();
}
