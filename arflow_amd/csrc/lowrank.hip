// The low-rank covariance family on the pixel grid: the reparameterised sampler of
// losses/uflow_elbo_loss.py:180-188 and the Gram log-determinants of its entropy (:362-381), with their gradients.
//   std [B, 2R, M, N]: channel 2k + c is column k of flow component c in {0, 1}; 1 <= R <= 16; p = y N + x.
//   sampler:  Z[sB+b,c,p] = mean[b,c,p] + sum_k std[b,2k+c,p] eps[sB+b,2k+c]        eps [S B][2R]: one scalar per sample and column
//   entropy:  logdet[b,c] = log det G,  G[b,c] = U U^T,  U = std[b, c::2] as [R, M N];  ginv[b,c] = G^-1
//   backward: gmean[b,c,p]    = sum_s gZ[sB+b,c,p]
//             gstd[b,2i+c,p]  = sum_s eps[sB+b,2i+c] gZ[sB+b,c,p] + 2 glogdet[b,c] sum_j ginv[b,c,i,j] std[b,2j+c,p]
// Sampler and backward: one thread = one pixel of one (b, c); it loads its R coefficients ONCE and keeps them in registers for
// all S samples (the reference repeats std S-fold in memory).  Forward order per element: acc = mean, acc += RN(std_k eps_k) in k
// order (-ffp-contract=off keeps the products unfused).  Backward: the sums over s, then over j, in index order in the thread.
// Log-det, two launches in one call:
//   stage 1  a workgroup reduces CHUNK consecutive pixels of one (b, c) to a partial Gram in float64 (the product of two fp32
//            values is exact there) with v_mfma_f64_16x16x4_f64: for a Gram matrix the A and the B fragment of a lane are the SAME
//            value U[lane & 15][p + (lane >> 4)], rows >= R are fed zeros; the four waves' accumulators are added in wave order
//            through LDS and the R x R partial goes to the work buffer [B][2][chunks][R][R].
//   stage 2  one wave per (b, c) adds the partials in chunk order, factors G = L L^T in float64, and writes
//            logdet = 2 sum_i log L_ii and G^-1 = L^-T L^-1 rounded once to fp32.  A pivot that is not positive (G singular or
//            indefinite to working precision) makes that (b, c)'s logdet and ginv NaN -- no host synchronisation; the
//            reference's torch.logdet gives -inf / NaN there.
// No atomics anywhere: the same code and the same bits in normal and deterministic mode.  Every element of every output is
// stored.
#include "common.hpp"

namespace {

constexpr int RMAX = 16;
constexpr int NT = 256;           // threads of a workgroup: sampler, backward and stage 1 (4 waves)
constexpr int WAVE_PIX = 32;      // pixels one wave feeds per trip: two groups of 16 (a float4 per lane each)
constexpr int TRIPS = 8;
constexpr int CHUNK = (NT / AF_WAVE) * WAVE_PIX * TRIPS;  // 1024 pixels per stage-1 workgroup

typedef double double4_t __attribute__((ext_vector_type(4)));

// grid (ceil(M N / NT), 2 B)
__global__ __launch_bounds__(NT) void lowrank_sample_kernel(const float* __restrict__ mean, long mean_bs,
                                                            const float* __restrict__ std, long std_bs,
                                                            const float* __restrict__ eps, float* __restrict__ Z, long z_bs,
                                                            int B, int S, int R, long plane) {
  const long p = (long)blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y >> 1, c = blockIdx.y & 1;
  float a[RMAX];
#pragma unroll
  for (int k = 0; k < RMAX; ++k) a[k] = k < R ? std[b * std_bs + (2 * k + c) * plane + p] : 0.f;
  const float mu = mean[b * mean_bs + c * plane + p];
  for (int s = 0; s < S; ++s) {
    const long sp = (long)s * B + b;
    const float* e = eps + sp * 2 * R + c;
    float acc = mu;
#pragma unroll
    for (int k = 0; k < RMAX; ++k)
      if (k < R) {
        const float term = a[k] * e[2 * k];
        acc += term;
      }
    Z[sp * z_bs + c * plane + p] = acc;
  }
}

// grid as the sampler.  gZ / glogdet may be NULL (that source is absent), gmean may be NULL (not wanted).
__global__ __launch_bounds__(NT) void lowrank_bwd_kernel(const float* __restrict__ std, long std_bs,
                                                         const float* __restrict__ eps, const float* __restrict__ gZ,
                                                         long gz_bs, const float* __restrict__ ginv,
                                                         const float* __restrict__ glogdet, float* __restrict__ gmean,
                                                         long gmean_bs, float* __restrict__ gstd, long gstd_bs, int B, int S,
                                                         int R, long plane) {
  const long p = (long)blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y >> 1, c = blockIdx.y & 1;
  float ga[RMAX];
#pragma unroll
  for (int k = 0; k < RMAX; ++k) ga[k] = 0.f;
  float gm = 0.f;
  if (gZ) {
    for (int s = 0; s < S; ++s) {
      const long sp = (long)s * B + b;
      const float g = gZ[sp * gz_bs + c * plane + p];
      const float* e = eps + sp * 2 * R + c;
      gm += g;
#pragma unroll
      for (int k = 0; k < RMAX; ++k)
        if (k < R) {
          const float term = e[2 * k] * g;
          ga[k] += term;
        }
    }
  }
  if (gmean) gmean[b * gmean_bs + c * plane + p] = gm;
  if (glogdet) {
    float u[RMAX];
#pragma unroll
    for (int k = 0; k < RMAX; ++k) u[k] = k < R ? std[b * std_bs + (2 * k + c) * plane + p] : 0.f;
    const float two_g = 2.f * glogdet[2 * b + c];
    const float* gi = ginv + (long)(2 * b + c) * R * R;
#pragma unroll
    for (int i = 0; i < RMAX; ++i)
      if (i < R) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < RMAX; ++j)
          if (j < R) {
            const float term = gi[i * R + j] * u[j];
            t += term;
          }
        const float second = two_g * t;
        ga[i] += second;
      }
  }
#pragma unroll
  for (int k = 0; k < RMAX; ++k)
    if (k < R) gstd[b * gstd_bs + (2 * k + c) * plane + p] = ga[k];
}

// Stage 1.  grid (chunks, 2 B).  VEC: float4 loads (M N % 4 == 0 and every plane of std 16-byte aligned, host-checked).
template <bool VEC>
__global__ __launch_bounds__(NT) void lowrank_gram_kernel(const float* __restrict__ std, long std_bs,
                                                          double* __restrict__ work, int R, long plane) {
  __shared__ double part[NT / AF_WAVE][RMAX * RMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y >> 1, c = blockIdx.y & 1;
  const int row = lane & 15, grp = lane >> 4;  // the lane's row of U, and which 4 pixels of a group of 16 it loads
  const float* u = std + b * std_bs + (2L * row + c) * plane;
  const long p0 = (long)blockIdx.x * CHUNK + wave * WAVE_PIX + 4 * grp;
  double4_t acc = {0., 0., 0., 0.};
  for (int t = 0; t < TRIPS; ++t) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const long p = p0 + (long)t * (NT / AF_WAVE) * WAVE_PIX + 16 * half;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < R) {
        if (VEC) {
          if (p < plane) v = *reinterpret_cast<const float4*>(u + p);  // plane % 4 == 0: a group is inside or outside
        } else {
          if (p + 0 < plane) v.x = u[p + 0];
          if (p + 1 < plane) v.y = u[p + 1];
          if (p + 2 < plane) v.z = u[p + 2];
          if (p + 3 < plane) v.w = u[p + 3];
        }
      }
      // each MFMA adds 4 pixels (one per lane group) to all 16 x 16 entries; which pixel goes into which is free
      const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(z, z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w, w, acc, 0, 0, 0);
    }
  }
  // f64 C/D map: register r of a lane is entry (row (lane >> 4) + 4 r, column lane & 15)
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][(grp + 4 * r) * RMAX + row] = acc[r];
  __syncthreads();
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  if (i < R && j < R) {
    double s = part[0][i * RMAX + j];
#pragma unroll
    for (int w = 1; w < NT / AF_WAVE; ++w) s += part[w][i * RMAX + j];
    work[((long)blockIdx.y * gridDim.x + blockIdx.x) * R * R + i * R + j] = s;
  }
}

// Stage 2.  grid (2 B), one wave.
__global__ __launch_bounds__(AF_WAVE) void lowrank_factor_kernel(const double* __restrict__ work, int chunks,
                                                                 float* __restrict__ logdet, float* __restrict__ ginv,
                                                                 int R) {
  __shared__ double L[RMAX][RMAX + 1];   // G, then its Cholesky factor in the lower triangle
  __shared__ double Li[RMAX][RMAX + 1];  // L^-1 (lower triangle, zeros above)
  __shared__ double rdiag[RMAX];         // 1 / L_ii
  const int lane = threadIdx.x;
  const int bc = blockIdx.x;
  const double* w = work + (long)bc * chunks * R * R;
  for (int e = lane; e < R * R; e += AF_WAVE) {
    double s = 0.;
    for (int q = 0; q < chunks; ++q) s += w[(long)q * R * R + e];  // in chunk order
    L[e / R][e % R] = s;
  }
  __syncthreads();
  // left-looking, lane i = row i: column j reads the finished columns k < j and its own entry of G, and writes column j only
  bool bad = false;
  for (int j = 0; j < R; ++j) {
    double v = 0.;
    if (lane >= j && lane < R) {
      v = L[lane][j];
      for (int k = 0; k < j; ++k) v -= L[lane][k] * L[j][k];
    }
    const double d2 = __shfl(v, j, AF_WAVE);  // the pivot, from lane j
    if (!(d2 > 0.)) bad = true;
    const double d = sqrt(d2);
    if (lane == j) {
      L[j][j] = d;
      rdiag[j] = 1. / d;
    } else if (lane > j && lane < R) {
      L[lane][j] = v / d;
    }
    __syncthreads();
  }
  const double lg = lane < R ? log(L[lane][lane]) : 0.;
  double sumlog = 0.;
  for (int i = 0; i < R; ++i) sumlog += __shfl(lg, i, AF_WAVE);  // in index order
  // column `lane` of L^-1 by forward substitution, in registers (zero above the diagonal)
  double x[RMAX];
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    x[i] = 0.;
    if (i < R) {
      double s = i == lane ? 1. : 0.;
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * x[k];
      x[i] = s * rdiag[i];
    }
  }
  if (lane < R) {
#pragma unroll
    for (int i = 0; i < RMAX; ++i)
      if (i < R) Li[i][lane] = x[i];
  }
  __syncthreads();
  const float nan = __builtin_nanf("");
  for (int e = lane; e < R * R; e += AF_WAVE) {
    const int i = e / R, j = e % R;
    double s = 0.;
    for (int k = (i > j ? i : j); k < R; ++k) s += Li[k][i] * Li[k][j];
    ginv[(long)bc * R * R + e] = bad ? nan : (float)s;
  }
  if (lane == 0) logdet[bc] = bad ? nan : (float)(2. * sumlog);
}


inline int check_dims(int B, int S, int R, int M, int N) {
  AF_REQUIRE(R >= 1 && R <= RMAX, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && S >= 1 && M >= 1 && N >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE((long)M * N <= 0x7fffffffL && (long)S * B <= 0x7fffffffL, ARFLOW_ESHAPE);
  AF_REQUIRE(2L * B <= 65535, ARFLOW_ESHAPE);  // gridDim.y
  return ARFLOW_OK;
}

}  // namespace

extern "C" int arflow_lowrank_sample_fwd(const float* mean, long mean_bs, const float* std, long std_bs, const float* eps,
                                         float* Z, long z_bs, int B, int S, int R, int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(mean);
  AF_REQUIRE_PTR(std);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(Z);
  const int rc = check_dims(B, S, R, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N;
  AF_REQUIRE(af_stride_ok(mean_bs, B, 2 * plane) && af_stride_ok(std_bs, B, 2L * R * plane) &&
                 af_stride_ok(z_bs, (long)S * B, 2 * plane),
             ARFLOW_ESHAPE);
  hipLaunchKernelGGL(lowrank_sample_kernel, dim3(af_cdiv(plane, NT), 2 * B), dim3(NT), 0, (hipStream_t)stream, mean, mean_bs,
                     std, std_bs, eps, Z, z_bs, B, S, R, plane);
  return af_launch_status();
}

extern "C" long arflow_lowrank_work_size(int B, int R, int M, int N) {
  if (R < 1 || R > RMAX) return ARFLOW_EPARAM;
  if (B < 1 || M < 1 || N < 1 || (long)M * N > 0x7fffffffL || 2L * B > 65535) return ARFLOW_ESHAPE;
  return 2L * B * af_cdiv((long)M * N, CHUNK) * R * R;
}

extern "C" int arflow_lowrank_logdet_fwd(const float* std, long std_bs, double* work, float* logdet, float* ginv, int B, int R,
                                         int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(std);
  AF_REQUIRE_PTR(work);
  AF_REQUIRE_PTR(logdet);
  AF_REQUIRE_PTR(ginv);
  const int rc = check_dims(B, 1, R, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N;
  AF_REQUIRE(af_stride_ok(std_bs, B, 2L * R * plane), ARFLOW_ESHAPE);
  const int chunks = af_cdiv(plane, CHUNK);
  const bool vec = plane % 4 == 0 && af_vec4_ok(std, std_bs, B);
  const dim3 grid(chunks, 2 * B);
  if (vec)
    hipLaunchKernelGGL(lowrank_gram_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, std, std_bs, work, R, plane);
  else
    hipLaunchKernelGGL(lowrank_gram_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, std, std_bs, work, R, plane);
  AF_LAUNCH_CHECK();
  hipLaunchKernelGGL(lowrank_factor_kernel, dim3(2 * B), dim3(AF_WAVE), 0, (hipStream_t)stream, work, chunks, logdet, ginv, R);
  return af_launch_status();
}

extern "C" int arflow_lowrank_bwd(const float* std, long std_bs, const float* eps, const float* gZ, long gz_bs,
                                  const float* ginv, const float* glogdet, float* gmean, long gmean_bs, float* gstd,
                                  long gstd_bs, int B, int S, int R, int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(std);
  AF_REQUIRE_PTR(gstd);
  if (gZ) AF_REQUIRE_PTR(eps);
  if (glogdet) AF_REQUIRE_PTR(ginv);
  const int rc = check_dims(B, S, R, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N;
  AF_REQUIRE(af_stride_ok(std_bs, B, 2L * R * plane) && af_stride_ok(gstd_bs, B, 2L * R * plane) &&
                 (!gZ || af_stride_ok(gz_bs, (long)S * B, 2 * plane)) && (!gmean || af_stride_ok(gmean_bs, B, 2 * plane)),
             ARFLOW_ESHAPE);
  hipLaunchKernelGGL(lowrank_bwd_kernel, dim3(af_cdiv(plane, NT), 2 * B), dim3(NT), 0, (hipStream_t)stream, std, std_bs, eps,
                     gZ, gz_bs, ginv, glogdet, gmean, gmean_bs, gstd, gstd_bs, B, S, R, plane);
  return af_launch_status();
}
