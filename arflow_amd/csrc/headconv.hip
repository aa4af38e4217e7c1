// Direct 3x3 convolution with TWO output channels (stride 1, padding 1), all three passes, for gfx950: the flow heads of
// the host models (FlowEstimatorDense.conv_last 595->2 / 563->2, FlowEstimatorReduce.predict_flow, the last conv of
// ContextNetwork 32->2; models/pwclite.py:48-106).  MIOpen has no kernel for an output two channels wide and pads it
// into 32-wide Winograd / implicit-GEMM tiles; the problem itself is one pass over the wide tensor (x forward and for
// the weight gradient, dx for the data gradient) with 18 multiply-adds per element, i.e. HBM-bound.
//
// Common shape of the three kernels: a lane owns a STRIP of R rows x 4 columns of the wide tensor's plane (strips are
// numbered linearly over (sample, row group, column group), so consecutive lanes touch consecutive float4 of a row) and
// keeps the (R+2) x 6 neighbourhood of the narrow side in registers; the 18 weights of a channel are wave-uniform
// (scalar loads).  Every sum has a fixed order: no atomics, results are bitwise reproducible.
//
// Every multiply-add accumulates in DOUBLE and is rounded to fp32 once, at the store.  For small problems the vendor
// library runs naive kernels with double accumulators, so an fp32 chain of 18 (data gradient) or 9 C + 1 (forward) terms
// is up to ~4x further from the exact result than what these layers used to run; with double sums the result is the
// correctly rounded one (up to double rounding) for every shape.  The price, measured at 16x595x96x160: forward / data /
// weight gradient 320 / 200 / 195 us instead of 281 / 132 / 156 us with fp32 chains.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "common.hpp"

namespace {
constexpr int NT = 256;         // data / weight gradient: 4 waves, each on its own 64 strips
// forward: the waves of a workgroup share 64 strips and split the channels; strips of 2 and 4 rows need more than the 128 VGPRs
// a 16-wave workgroup leaves a lane
constexpr int fwd_max_waves(int R) { return R >= 2 ? 8 : 16; }

// Where a lane's strip lies: sample, first row, first column; `active` false for the padding lanes of the last wave
// (they are clamped onto the last strip so that every address stays in bounds, and neither store nor contribute).
template <int R>
struct Strip {
  int b, r0, q0;
  bool active;
  __device__ __forceinline__ Strip(long id, long nstrips, int H, int W) {
    active = id < nstrips;
    if (!active) id = nstrips - 1;
    const int w4 = (W + 3) >> 2, rg = (H + R - 1) / R;
    q0 = 4 * (int)(id % w4);
    r0 = R * (int)((id / w4) % rg);
    b = (int)(id / ((long)w4 * rg));
  }
};

// Addressing of the (R+2) x 6 neighbourhood rows r0-1 .. r0+R, columns q0-1 .. q0+4 of a plane, zero outside the plane.
// ALIGNED (W % 4 == 0, 16-byte aligned base): one float4 and the two halo columns per row; otherwise six guarded scalars.
template <int R, bool ALIGNED>
struct Nbhd {
  int ro[R + 2];    // offset of (clamped row, q0)
  bool rok[R + 2];  // row inside the plane
  int co[6];        // clamped column - q0
  bool cok[6];
  __device__ __forceinline__ Nbhd(int r0, int q0, int H, int W, bool active) {
#pragma unroll
    for (int i = 0; i < R + 2; ++i) {
      const int r = r0 - 1 + i;
      rok[i] = active && r >= 0 && r < H;
      ro[i] = min(max(r, 0), H - 1) * W + q0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int q = q0 - 1 + j;
      cok[j] = q >= 0 && q < W;
      co[j] = min(max(q, 0), W - 1) - q0;
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ plane, float (&v)[R + 2][6]) const {
#pragma unroll
    for (int i = 0; i < R + 2; ++i) {
      const float* p = plane + ro[i];
      if (ALIGNED) {
        const float4 m = *reinterpret_cast<const float4*>(p);
        const float l = p[co[0]], r = p[co[5]];
        v[i][0] = (rok[i] && cok[0]) ? l : 0.f;
        v[i][1] = rok[i] ? m.x : 0.f;
        v[i][2] = rok[i] ? m.y : 0.f;
        v[i][3] = rok[i] ? m.z : 0.f;
        v[i][4] = rok[i] ? m.w : 0.f;
        v[i][5] = (rok[i] && cok[5]) ? r : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float t = p[co[j]];
          v[i][j] = (rok[i] && cok[j]) ? t : 0.f;
        }
      }
    }
  }
};

// The R x 4 strip itself (no halo): offsets and validity of its rows / columns.
template <int R, bool ALIGNED>
struct Own {
  int ro[R];
  bool rok[R];
  bool cok[4];
  __device__ __forceinline__ Own(int r0, int q0, int H, int W, bool active) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      rok[a] = active && r0 + a < H;
      ro[a] = min(r0 + a, H - 1) * W + q0;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) cok[e] = q0 + e < W;
  }
  __device__ __forceinline__ void store(float* __restrict__ plane, int a, const float (&v)[4]) const {
    if (!rok[a]) return;
    float* p = plane + ro[a];
    if (ALIGNED) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (cok[e]) p[e] = v[e];
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ plane, float (&v)[R][4]) const {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const float* p = plane + ro[a];
      if (ALIGNED) {
        const float4 m = *reinterpret_cast<const float4*>(p);
        v[a][0] = rok[a] ? m.x : 0.f, v[a][1] = rok[a] ? m.y : 0.f, v[a][2] = rok[a] ? m.z : 0.f, v[a][3] = rok[a] ? m.w : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = p[cok[e] ? e : 0];
          v[a][e] = (rok[a] && cok[e]) ? t : 0.f;
        }
      }
    }
  }
};

// both dy neighbourhoods of a strip, widened once
template <int R, bool ALIGNED>
__device__ __forceinline__ void load_dy(const Nbhd<R, ALIGNED>& nb, const float* __restrict__ dy0, long HW, double (&d)[2][R + 2][6]) {
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    float t[R + 2][6];
    nb.load(dy0 + o * HW, t);
#pragma unroll
    for (int i = 0; i < R + 2; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) d[o][i][j] = (double)t[i][j];
  }
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// ---- forward ------------------------------------------------------------------------------------------------------------
// y[b,o,r,q] = bias[o] + sum_c sum_ky,kx w[o,c,ky,kx] x[b,c,r+ky-1,q+kx-1].  All waves of a workgroup own the SAME 64 strips
// and each takes a contiguous slice of the channels (at 96x160x16 the strips alone are only a few hundred waves); the
// slices are then added pairwise through LDS in a fixed tree, wave 0 (which started from the bias) stores.
template <int R, bool ALIGNED>
__global__ __launch_bounds__(64 * fwd_max_waves(R)) void headconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                           const float* __restrict__ bias, float* __restrict__ y,
                                                                           int C, int H, int W, long nstrips, int c_per_wave) {
  extern __shared__ __align__(16) double comb[];  // [nwaves / 2][2 * R * 4][64]
  const int lane = threadIdx.x & 63, wv = wave_id(), nw = blockDim.x >> 6;
  const Strip<R> s((long)blockIdx.x * 64 + lane, nstrips, H, W);
  const Nbhd<R, ALIGNED> nb(s.r0, s.q0, H, W, s.active);
  const long HW = (long)H * W;
  double acc[2][R][4];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const double b0 = (wv == 0 && bias) ? (double)bias[o] : 0.0;
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[o][a][e] = b0;
  }
  const int cbeg = min(wv * c_per_wave, C), cend = min(cbeg + c_per_wave, C);
  const float* xs = x + (long)s.b * C * HW;
  float nx[R + 2][6];  // the next channel's neighbourhood, in flight while this one is multiplied
  if (cbeg < cend) nb.load(xs + cbeg * HW, nx);
  for (int c = cbeg; c < cend; ++c) {
    double v[R + 2][6];
#pragma unroll
    for (int i = 0; i < R + 2; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) v[i][j] = (double)nx[i][j];
    nb.load(xs + min(c + 1, cend - 1) * HW, nx);
    const float* w0 = w + (long)c * 9;
    const float* w1 = w + ((long)C + c) * 9;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const double a0 = (double)w0[ky * 3 + kx], a1 = (double)w1[ky * 3 + kx];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[0][a][e] = fma(a0, v[a + ky][e + kx], acc[0][a][e]);
            acc[1][a][e] = fma(a1, v[a + ky][e + kx], acc[1][a][e]);
          }
      }
  }
  for (int h = nw >> 1; h >= 1; h >>= 1) {  // waves [h, 2h) hand their sums to waves [0, h)
    if (wv >= h && wv < 2 * h) {
      double* dst = comb + (long)(wv - h) * (2 * R * 4 * 64) + lane;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e) dst[((o * R + a) * 4 + e) * 64] = acc[o][a][e];
    }
    __syncthreads();
    if (wv < h) {
      const double* src = comb + (long)wv * (2 * R * 4 * 64) + lane;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[o][a][e] += src[((o * R + a) * 4 + e) * 64];
    }
    __syncthreads();
  }
  if (wv == 0) {
    const Own<R, ALIGNED> own(s.r0, s.q0, H, W, s.active);
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const float r[4] = {(float)acc[o][a][0], (float)acc[o][a][1], (float)acc[o][a][2], (float)acc[o][a][3]};
        own.store(y + ((long)s.b * 2 + o) * HW, a, r);
      }
  }
}

// ---- data gradient ------------------------------------------------------------------------------------------------------
// dx[b,c,r,q] = sum_o sum_ky,kx w[o,c,ky,kx] dy[b,o,r-ky+1,q-kx+1]: the lane keeps both dy neighbourhoods of its strip and
// writes dx channel by channel (grid.y splits the channels), a pure store stream.
template <int R, bool ALIGNED>
__global__ __launch_bounds__(NT) void headconv_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int C, int H, int W, long nstrips,
                                                               int c_per_block) {
  const Strip<R> s((long)blockIdx.x * NT + threadIdx.x, nstrips, H, W);
  const Nbhd<R, ALIGNED> nb(s.r0, s.q0, H, W, s.active);
  const Own<R, ALIGNED> own(s.r0, s.q0, H, W, s.active);
  const long HW = (long)H * W;
  double d[2][R + 2][6];
  load_dy(nb, dy + ((long)s.b * 2) * HW, HW, d);
  const int cbeg = blockIdx.y * c_per_block, cend = min(cbeg + c_per_block, C);
  float* dxs = dx + (long)s.b * C * HW;
  for (int c = cbeg; c < cend; ++c) {
    double wt[2][9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[0][t] = (double)w[(long)c * 9 + t], wt[1][t] = (double)w[((long)C + c) * 9 + t];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fma(wt[o][ky * 3 + kx], d[o][a + 2 - ky][e + 2 - kx], r[e]);
      const float rf[4] = {(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
      own.store(dxs + c * HW, a, rf);
    }
  }
}

// ---- weight and bias gradient -------------------------------------------------------------------------------------------
// dw[o,c,ky,kx] = sum_b,r,q dy[b,o,r-ky+1,q-kx+1] x[b,c,r,q].  A lane owns a strip of x and keeps both dy neighbourhoods;
// per channel it accumulates its 18 products over the strip, the wave adds them up with a transposing butterfly (each
// exchange halves the values a lane holds: 21 exchanges for 18 sums instead of 108) and stores one partial per
// (channel, weight, wave) into the workspace; headconv_finish_kernel adds the partials in a fixed order.
// Workspace: double part[C][18][G] then dpart[2][G] (partial sums of dy for dbias), G = number of 64-strip groups.
template <int N>
__device__ __forceinline__ void halve(double (&a)[18], int lane, int bit) {  // N values -> (N + 1) / 2, partner = lane ^ bit
  constexpr int M = (N + 1) / 2;
  const bool up = lane & bit;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const double hi = i + M < N ? a[i + M] : 0.0;
    const double keep = up ? hi : a[i], send = up ? a[i] : hi;
    a[i] = keep + __shfl_xor(send, bit, 64);
  }
}

template <int R, bool ALIGNED>
__global__ __launch_bounds__(NT) void headconv_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 double* __restrict__ part, double* __restrict__ dpart, int C, int H,
                                                                 int W, long nstrips, int G, int c_per_block) {
  const int lane = threadIdx.x & 63;
  const int grp = blockIdx.x * (NT / 64) + wave_id();
  if (grp >= G) return;
  const Strip<R> s((long)grp * 64 + lane, nstrips, H, W);
  const Nbhd<R, ALIGNED> nb(s.r0, s.q0, H, W, s.active);
  const Own<R, ALIGNED> own(s.r0, s.q0, H, W, s.active);
  const long HW = (long)H * W;
  double d[2][R + 2][6];
  load_dy(nb, dy + ((long)s.b * 2) * HW, HW, d);
  if (blockIdx.y == 0) {  // dbias: the strip's own dy (rows beyond H / columns beyond W of the neighbourhood are zero)
    double sb[2] = {0.0, 0.0};
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) sb[o] += d[o][a + 1][e + 1];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sb[0] += __shfl_xor(sb[0], off, 64), sb[1] += __shfl_xor(sb[1], off, 64);
    if (lane == 0) dpart[grp] = sb[0], dpart[G + grp] = sb[1];
  }
  // after the butterfly lane L (even) holds weight index k(L), see halve(): 18 -> 9 -> 5 -> 3 -> 2 -> 1
  const int i1 = (lane >> 1) & 1, i2 = 2 * ((lane >> 2) & 1) + i1, i3 = 3 * ((lane >> 3) & 1) + i2,
            i4 = 5 * ((lane >> 4) & 1) + i3, k = 9 * ((lane >> 5) & 1) + i4;
  const bool writer = !(lane & 1) && i2 < 3 && i3 < 5 && i4 < 9;
  const int cbeg = blockIdx.y * c_per_block, cend = min(cbeg + c_per_block, C);
  const float* xs = x + (long)s.b * C * HW;
  float nx[R][4];  // the next channel's strip, in flight while this one is multiplied
  if (cbeg < cend) own.load(xs + cbeg * HW, nx);
  for (int c = cbeg; c < cend; ++c) {
    double v[R][4];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[a][e] = (double)nx[a][e];
    own.load(xs + min(c + 1, cend - 1) * HW, nx);
    double acc[18];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) t = fma(v[a][e], d[o][a + 2 - ky][e + 2 - kx], t);
          acc[o * 9 + ky * 3 + kx] = t;
        }
    halve<18>(acc, lane, 32);
    halve<9>(acc, lane, 16);
    halve<5>(acc, lane, 8);
    halve<3>(acc, lane, 4);
    halve<2>(acc, lane, 2);
    acc[0] += __shfl_xor(acc[0], 1, 64);
    if (writer) part[((long)c * 18 + k) * G + grp] = acc[0];
  }
}

// One wave per (channel, weight) pair, and one per bias: G partials added lane-strided, then a butterfly.
__global__ __launch_bounds__(NT) void headconv_finish_kernel(const double* __restrict__ part, const double* __restrict__ dpart,
                                                             float* __restrict__ dw, float* __restrict__ dbias, int C, int G) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * (NT / 64) + wave_id();
  const long nw = (long)C * 18;
  if (item >= nw + (dbias ? 2 : 0)) return;
  const double* src = item < nw ? part + item * G : dpart + (item - nw) * G;
  double t = 0.0;
  for (int g = lane; g < G; g += 64) t += src[g];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
  if (lane == 0) {
    if (item < nw) {
      const int c = (int)(item / 18), k = (int)(item % 18);
      dw[((long)(k / 9) * C + c) * 9 + k % 9] = (float)t;
    } else {
      dbias[item - nw] = (float)t;
    }
  }
}

constexpr int WG_R = 4;  // rows per strip of the weight gradient
constexpr int DG_R = 2;  // rows per strip of the data gradient (1 and 4 measured 15 % slower)

inline long strips(int B, int H, int W, int R) { return (long)B * ((H + R - 1) / R) * ((W + 3) / 4); }
inline bool shape_ok(int B, int C, int H, int W) {
  return B > 0 && C > 0 && H > 0 && W > 0 && (long)H * W <= INT_MAX / 2 && (long)C * 18 < INT_MAX / 4 &&
         strips(B, H, W, 1) / 64 < INT_MAX / 2 && C <= 65535 * 4;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// channels per grid.y slice: enough slices for ~4096 waves, at least 4 channels each
inline int channels_per_block(long waves, int C) {
  long nch = (4096 + waves - 1) / waves;
  nch = std::max(1L, std::min(nch, (long)(C + 3) / 4));
  return (int)((C + nch - 1) / nch);
}
}  // namespace

extern "C" int arflow_headconv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W,
                                   arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(w);
  AF_REQUIRE_PTR(y);
  AF_REQUIRE(shape_ok(B, C, H, W), ARFLOW_ESHAPE);
  // rows per strip: the tallest strip that still gives every CU a workgroup (a taller strip re-reads fewer halo rows)
  // (measured at the flagship shapes: 50 or 100 instead of 200 cost 2-3x at 48x80)
  int R = 4;
  while (R > 1 && (strips(B, H, W, R) + 63) / 64 < 200) R >>= 1;
  int nw = 1;  // waves per workgroup = channel slices, at least 8 channels each
  while (nw < fwd_max_waves(R) && nw * 2 * 8 <= C) nw *= 2;
  const int cpw = (C + nw - 1) / nw;
  const long ns = strips(B, H, W, R);
  const dim3 grid((unsigned)((ns + 63) / 64)), block(64 * nw);
  const size_t lds = (size_t)(nw / 2) * 2 * R * 4 * 64 * sizeof(double);
  const bool al = (W & 3) == 0 && aligned16(x) && aligned16(y);
  hipStream_t st = (hipStream_t)stream;
#define AF_HEAD_FWD(R_, A_) \
  hipLaunchKernelGGL((headconv_fwd_kernel<R_, A_>), grid, block, lds, st, x, w, bias, y, C, H, W, ns, cpw)
  if (R == 4) {
    if (al) AF_HEAD_FWD(4, true); else AF_HEAD_FWD(4, false);
  } else if (R == 2) {
    if (al) AF_HEAD_FWD(2, true); else AF_HEAD_FWD(2, false);
  } else {
    if (al) AF_HEAD_FWD(1, true); else AF_HEAD_FWD(1, false);
  }
#undef AF_HEAD_FWD
  return af_launch_status();
}

extern "C" int arflow_headconv_bwd_data(const float* dy, const float* w, float* dx, int B, int C, int H, int W,
                                        arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(dy);
  AF_REQUIRE_PTR(w);
  AF_REQUIRE_PTR(dx);
  AF_REQUIRE(shape_ok(B, C, H, W), ARFLOW_ESHAPE);
  const long ns = strips(B, H, W, DG_R);
  const unsigned gx = (unsigned)((ns + NT - 1) / NT);
  const int cpb = channels_per_block((long)gx * (NT / 64), C);
  const dim3 grid(gx, (unsigned)((C + cpb - 1) / cpb));
  const bool al = (W & 3) == 0 && aligned16(dy) && aligned16(dx);
  hipStream_t st = (hipStream_t)stream;
  if (al)
    hipLaunchKernelGGL((headconv_bwd_data_kernel<DG_R, true>), grid, dim3(NT), 0, st, dy, w, dx, C, H, W, ns, cpb);
  else
    hipLaunchKernelGGL((headconv_bwd_data_kernel<DG_R, false>), grid, dim3(NT), 0, st, dy, w, dx, C, H, W, ns, cpb);
  return af_launch_status();
}

extern "C" long arflow_headconv_bwd_weight_ws_bytes(int B, int C, int H, int W) {
  if (!shape_ok(B, C, H, W)) return ARFLOW_ESHAPE;
  const long G = (strips(B, H, W, WG_R) + 63) / 64;
  return (long)sizeof(double) * G * ((long)C * 18 + 2);
}

extern "C" int arflow_headconv_bwd_weight(const float* x, const float* dy, float* dw, float* dbias, void* ws, int B, int C,
                                          int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(dy);
  AF_REQUIRE_PTR(dw);
  AF_REQUIRE_PTR(ws);
  AF_REQUIRE(shape_ok(B, C, H, W), ARFLOW_ESHAPE);
  AF_REQUIRE(aligned16(ws), ARFLOW_EPARAM);
  const long ns = strips(B, H, W, WG_R);
  const int G = (int)((ns + 63) / 64);
  double* part = (double*)ws;
  double* dpart = part + (long)C * 18 * G;
  const unsigned gx = (unsigned)((G + NT / 64 - 1) / (NT / 64));
  const int cpb = channels_per_block(G, C);
  const dim3 grid(gx, (unsigned)((C + cpb - 1) / cpb));
  const bool al = (W & 3) == 0 && aligned16(x) && aligned16(dy);
  hipStream_t st = (hipStream_t)stream;
  if (al)
    hipLaunchKernelGGL((headconv_bwd_weight_kernel<WG_R, true>), grid, dim3(NT), 0, st, x, dy, part, dpart, C, H, W, ns, G, cpb);
  else
    hipLaunchKernelGGL((headconv_bwd_weight_kernel<WG_R, false>), grid, dim3(NT), 0, st, x, dy, part, dpart, C, H, W, ns, G, cpb);
  AF_LAUNCH_CHECK();
  const long items = (long)C * 18 + (dbias ? 2 : 0);
  hipLaunchKernelGGL(headconv_finish_kernel, dim3((unsigned)((items + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, part, dpart,
                     dw, dbias, C, G);
  return af_launch_status();
}
