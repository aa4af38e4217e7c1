// The banded operator of the sparse-covariance family on the pixel grid: matrix_vector_product_general
// and matrix_vector_product_T_general of utils/triag_solve.py:29-43, :59-73, their gradients, and -- with S samples per batch
// item and a mean -- the reparameterised sampler z = mean + L eps of losses/uflow_elbo_loss.py:142-147.
//   k in 0..3, taps (i, j), 0 <= i, j <= k, ind = i (k + 1) + j; coefficient A[b, ind, c, y, x], c in {0, 1}: ind = 0 from
//   `diag` (2 channels per batch item), ind >= 1 from channel 2 (ind - 1) + c of `off` (2 ((k+1)^2 - 1) channels).
//   Sample s of batch item b is plane s B + b of X, Y, gY, gX (the reference's repeat(nsamples, 1, 1, 1) order).
//   plain:       Y[sB+b,c,y,x] = mean[b,c,y,x] + sum_ind A[b,ind,c,y-i,x-j] X[sB+b,c,y-i,x-j]     (y-i >= 0, x-j >= 0)
//   transposed:  Y[sB+b,c,y,x] = mean[b,c,y,x] + sum_ind A[b,ind,c,y,x]     X[sB+b,c,y+i,x+j]     (y+i < M,  x+j < N)
// One workgroup = one TH x TW tile of one (b, c) plane, one thread = one pixel, a wave = two rows of 32 consecutive floats.
// The thread loads its (k+1)^2 coefficients ONCE (row segments shifted by j: coalesced) and keeps them in registers for all
// S samples; per sample the X window of the tile with its k halo ((TH + k) x (TW + k)) goes through LDS, double-buffered so
// that a sample costs one barrier.  A wave reads a window row at consecutive addresses: no bank conflict at any row stride.
// Forward order per element, as the reference: acc = 0, acc += RN(A X) in ind order (a tap outside the grid adds +0, the
// reference's F.pad), then mean + acc; -ffp-contract=off keeps the products unfused, so both orientations give the bits of
// the reference's fp32 CPU run.
// Backward, one launch: with G = gY,
//   plain:       gX = transposed product of G;   gA[b,ind,c,y,x] = sum_s X[sB+b,c,y,x] G[sB+b,c,y+i,x+j]
//   transposed:  gX = plain product of G;        gA[b,ind,c,y,x] = sum_s G[sB+b,c,y,x] X[sB+b,c,y+i,x+j]
//   gmean[b] = sum_s G[sB+b]
// The sums over s and the taps run in a fixed order inside the pixel's thread: no atomics, the same code and bits in normal
// and deterministic mode.  Every element of every output is stored (a tap outside the grid contributes an exact 0).
#include "common.hpp"

namespace {

constexpr int TW = 32, TH = 8;      // tile: 8 rows of 32 pixels
constexpr int NT = TW * TH;         // threads of a workgroup (4 waves)
constexpr int KMAX = 3;
constexpr int WS = TW + KMAX;       // window row stride, floats
constexpr int WIN = (TH + KMAX) * WS;

// the (TH + K) x (TW + K) window whose first cell is grid cell (wy0, wx0) of plane `src`: global -> LDS, 0 outside the grid
template <int K>
__device__ __forceinline__ void stage(const float* __restrict__ src, float* __restrict__ w, int wy0, int wx0, int M, int N) {
  constexpr int WW = TW + K, WH = TH + K;
  for (int e = threadIdx.x; e < WW * WH; e += NT) {
    const int r = e / WW, q = e % WW;
    const int gy = wy0 + r, gx = wx0 + q;
    w[r * WS + q] = (gy >= 0 && gy < M && gx >= 0 && gx < N) ? src[(long)gy * N + gx] : 0.f;
  }
}

// the coefficient plane of tap `ind`, channel c, batch item b
__device__ __forceinline__ const float* coef(const float* diag, long diag_bs, const float* off, long off_bs, int b, int c,
                                             int ind, long plane) {
  return ind == 0 ? diag + b * diag_bs + c * plane : off + b * off_bs + (2 * (ind - 1) + c) * plane;
}
__device__ __forceinline__ float* coef(float* diag, long diag_bs, float* off, long off_bs, int b, int c, int ind, long plane) {
  return ind == 0 ? diag + b * diag_bs + c * plane : off + b * off_bs + (2 * (ind - 1) + c) * plane;
}

// grid (ceil(N / TW), ceil(M / TH), 2 B)
template <int K, int T>
__global__ __launch_bounds__(NT) void band_fwd_kernel(const float* __restrict__ mean, long mean_bs,
                                                      const float* __restrict__ diag, long diag_bs,
                                                      const float* __restrict__ off, long off_bs,
                                                      const float* __restrict__ X, long x_bs, float* __restrict__ Y,
                                                      long y_bs, int B, int S, int M, int N) {
  constexpr int NTAP = (K + 1) * (K + 1);
  __shared__ float win[2][WIN];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int b = blockIdx.z >> 1, c = blockIdx.z & 1;
  const int x = x0 + tx, y = y0 + ty;
  const bool in = x < N && y < M;
  const long plane = (long)M * N;
  const long own = (long)y * N + x;

  // plain: coefficient and X at the source pixel (y - i, x - j); transposed: coefficient at the pixel, X at (y + i, x + j)
  float a[NTAP];
  bool ok[NTAP];
#pragma unroll
  for (int i = 0; i <= K; ++i)
#pragma unroll
    for (int j = 0; j <= K; ++j) {
      const int ind = i * (K + 1) + j;
      const int sy = T ? y + i : y - i, sx = T ? x + j : x - j;
      ok[ind] = in && sy >= 0 && sy < M && sx >= 0 && sx < N;
      const long at = T ? own : (long)sy * N + sx;
      a[ind] = ok[ind] ? coef(diag, diag_bs, off, off_bs, b, c, ind, plane)[at] : 0.f;
    }
  const float mu = (mean && in) ? mean[b * mean_bs + c * plane + own] : 0.f;
  const int wy0 = T ? y0 : y0 - K, wx0 = T ? x0 : x0 - K;

  for (int s = 0; s < S; ++s) {
    float* w = win[s & 1];
    const long sp = (long)s * B + b;
    stage<K>(X + sp * x_bs + c * plane, w, wy0, wx0, M, N);
    __syncthreads();  // the other buffer is free again once every thread has passed the NEXT sample's barrier
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i <= K; ++i)
#pragma unroll
      for (int j = 0; j <= K; ++j) {
        const int ind = i * (K + 1) + j;
        const float xv = T ? w[(ty + i) * WS + tx + j] : w[(ty + K - i) * WS + tx + K - j];
        const float term = ok[ind] ? a[ind] * xv : 0.f;
        acc += term;
      }
    if (in) Y[sp * y_bs + c * plane + own] = mean ? mu + acc : acc;
  }
}

// grid as the forward.  T: the orientation of the FORWARD this is the backward of.
template <int K, int T>
__global__ __launch_bounds__(NT) void band_bwd_kernel(const float* __restrict__ diag, long diag_bs,
                                                      const float* __restrict__ off, long off_bs,
                                                      const float* __restrict__ X, long x_bs, const float* __restrict__ G,
                                                      long g_bs, float* __restrict__ gX, long gx_bs,
                                                      float* __restrict__ gmean, long gmean_bs, float* __restrict__ gdiag,
                                                      long gdiag_bs, float* __restrict__ goff, long goff_bs, int B, int S,
                                                      int M, int N) {
  constexpr int NTAP = (K + 1) * (K + 1);
  __shared__ float wing[2][WIN];
  __shared__ float winx[T ? 2 : 1][T ? WIN : 1];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int b = blockIdx.z >> 1, c = blockIdx.z & 1;
  const int x = x0 + tx, y = y0 + ty;
  const bool in = x < N && y < M;
  const long plane = (long)M * N;
  const long own = (long)y * N + x;

  // gX: the product of the OTHER orientation with the same coefficients; plus: the tap (y + i, x + j) is on the grid
  float a[NTAP], ga[NTAP];
  bool okx[NTAP], plus[NTAP];
#pragma unroll
  for (int i = 0; i <= K; ++i)
#pragma unroll
    for (int j = 0; j <= K; ++j) {
      const int ind = i * (K + 1) + j;
      plus[ind] = in && y + i < M && x + j < N;
      okx[ind] = T ? (in && y - i >= 0 && x - j >= 0) : plus[ind];
      const long at = T ? (long)(y - i) * N + (x - j) : own;
      a[ind] = okx[ind] ? coef(diag, diag_bs, off, off_bs, b, c, ind, plane)[at] : 0.f;
      ga[ind] = 0.f;
    }
  float gm = 0.f;
  // G window: plain forward -> taps at (+i, +j), first cell (y0, x0); transposed forward -> taps at (-i, -j)
  const int gy0 = T ? y0 - K : y0, gx0 = T ? x0 - K : x0;

  for (int s = 0; s < S; ++s) {
    float* wg = wing[s & 1];
    float* wx = winx[T ? (s & 1) : 0];
    const long sp = (long)s * B + b;
    stage<K>(G + sp * g_bs + c * plane, wg, gy0, gx0, M, N);
    if (T) stage<K>(X + sp * x_bs + c * plane, wx, y0, x0, M, N);
    const float xo = (!T && in) ? X[sp * x_bs + c * plane + own] : 0.f;
    __syncthreads();
    const float go = T ? wg[(ty + K) * WS + tx + K] : wg[ty * WS + tx];  // G at the pixel itself (0 outside the grid)
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i <= K; ++i)
#pragma unroll
      for (int j = 0; j <= K; ++j) {
        const int ind = i * (K + 1) + j;
        const float gv = T ? wg[(ty + K - i) * WS + tx + K - j] : wg[(ty + i) * WS + tx + j];
        acc += okx[ind] ? a[ind] * gv : 0.f;
        if (T)
          ga[ind] += plus[ind] ? go * wx[(ty + i) * WS + tx + j] : 0.f;
        else
          ga[ind] += plus[ind] ? xo * gv : 0.f;
      }
    gm += go;
    if (in && gX) gX[sp * gx_bs + c * plane + own] = acc;
  }
  if (!in) return;
  if (gmean) gmean[b * gmean_bs + c * plane + own] = gm;
#pragma unroll
  for (int ind = 0; ind < NTAP; ++ind) coef(gdiag, gdiag_bs, goff, goff_bs, b, c, ind, plane)[own] = ga[ind];
}

inline int check_dims(int B, int S, int M, int N) {
  AF_REQUIRE(B >= 1 && S >= 1 && M >= 1 && N >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE((long)M * N <= 0x7fffffffL && (long)S * B <= 0x7fffffffL, ARFLOW_ESHAPE);
  AF_REQUIRE(2L * B <= 65535 && af_cdiv(M, TH) <= 65535, ARFLOW_ESHAPE);  // gridDim.z, gridDim.y
  return ARFLOW_OK;
}
// a batch stride is read only when there is a second item

}  // namespace

#define BAND_DISPATCH(KERNEL, ...)                                                                                     \
  do {                                                                                                                 \
    const dim3 grid(af_cdiv(N, TW), af_cdiv(M, TH), 2 * B);                                                           \
    switch (k * 2 + transpose) {                                                                                       \
      case 0: hipLaunchKernelGGL((KERNEL<0, 0>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 1: hipLaunchKernelGGL((KERNEL<0, 1>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 2: hipLaunchKernelGGL((KERNEL<1, 0>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 3: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 4: hipLaunchKernelGGL((KERNEL<2, 0>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 5: hipLaunchKernelGGL((KERNEL<2, 1>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      case 6: hipLaunchKernelGGL((KERNEL<3, 0>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
      default: hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__); break;        \
    }                                                                                                                  \
  } while (0)

extern "C" int arflow_band_mv_fwd(const float* mean, long mean_bs, const float* diag, long diag_bs, const float* off,
                                  long off_bs, const float* X, long x_bs, float* Y, long y_bs, int B, int S, int M, int N,
                                  int k, int transpose, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(diag);
  AF_REQUIRE_PTR(X);
  AF_REQUIRE_PTR(Y);
  AF_REQUIRE(k >= 0 && k <= KMAX && (transpose == 0 || transpose == 1), ARFLOW_EPARAM);
  if (k > 0) AF_REQUIRE_PTR(off);
  const int rc = check_dims(B, S, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long pl = 2L * M * N, ntap = (long)(k + 1) * (k + 1);
  AF_REQUIRE(af_stride_ok(diag_bs, B, pl) && (k == 0 || af_stride_ok(off_bs, B, (ntap - 1) * pl)) &&
                 (!mean || af_stride_ok(mean_bs, B, pl)) && af_stride_ok(x_bs, (long)S * B, pl) &&
                 af_stride_ok(y_bs, (long)S * B, pl),
             ARFLOW_ESHAPE);
  BAND_DISPATCH(band_fwd_kernel, mean, mean_bs, diag, diag_bs, off, off_bs, X, x_bs, Y, y_bs, B, S, M, N);
  return af_launch_status();
}

extern "C" int arflow_band_mv_bwd(const float* diag, long diag_bs, const float* off, long off_bs, const float* X, long x_bs,
                                  const float* gY, long gy_bs, float* gX, long gx_bs, float* gmean, long gmean_bs,
                                  float* gdiag, long gdiag_bs, float* goff, long goff_bs, int B, int S, int M, int N, int k,
                                  int transpose, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(diag);
  AF_REQUIRE_PTR(X);
  AF_REQUIRE_PTR(gY);
  AF_REQUIRE_PTR(gdiag);
  AF_REQUIRE(k >= 0 && k <= KMAX && (transpose == 0 || transpose == 1), ARFLOW_EPARAM);
  if (k > 0) {
    AF_REQUIRE_PTR(off);
    AF_REQUIRE_PTR(goff);
  }
  const int rc = check_dims(B, S, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long pl = 2L * M * N, ntap = (long)(k + 1) * (k + 1);
  AF_REQUIRE(af_stride_ok(diag_bs, B, pl) && af_stride_ok(gdiag_bs, B, pl) &&
                 (k == 0 || (af_stride_ok(off_bs, B, (ntap - 1) * pl) && af_stride_ok(goff_bs, B, (ntap - 1) * pl))) &&
                 (!gmean || af_stride_ok(gmean_bs, B, pl)) && af_stride_ok(x_bs, (long)S * B, pl) &&
                 af_stride_ok(gy_bs, (long)S * B, pl) && (!gX || af_stride_ok(gx_bs, (long)S * B, pl)),
             ARFLOW_ESHAPE);
  BAND_DISPATCH(band_bwd_kernel, diag, diag_bs, off, off_bs, X, x_bs, gY, gy_bs, gX, gx_bs, gmean, gmean_bs, gdiag, gdiag_bs,
                goff, goff_bs, B, S, M, N);
  return af_launch_status();
}
