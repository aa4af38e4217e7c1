// The Gaussian-mixture variational family on the pixel grid: the sampler reparam_gmm of
// losses/uflow_elbo_loss.py:159-178, the mixture log-density of its entropy (utils/misc_utils.py:67-101, :358-361 of the
// loss) with their gradients, and the per-pixel Monte-Carlo entropy map (utils/misc_utils.py:104-132).
//   mean, log_std [B, 2K, M, N]: channel 2k + c is flow component c of mixture component k; 1 <= K <= 4; p = y N + x, P = M N.
//   weights [B, K] >= 0;  comp [B, S] (int64) in 0..K-1: the component sample s of item b is drawn from;  eps [S B, 2, M, N].
//   Sample s of item b is row n = s B + b;  z = comp[b, s];  std = exp(log_std).
//   sampler:  flow[n,c,p] = mean[b,2z+c,p] + std[b,2z+c,p] eps[n,c,p]
//   density:  d[n,k,c,p] = (flow[n,c,p] - mean[b,2k+c,p]) / std[b,2k+c,p]
//             A[n,k]     = - sum_p sum_c (log_std[b,2k+c,p] + d^2 / 2)
//             logpdf[n]  = (max_k A + log sum_k w[b,k] exp(A[n,k] - max_k A)) / P
//             resp[n,k]  = w[b,k] exp(A[n,k] - max) / sum_j w[b,j] exp(A[n,j] - max),   q[n,k] = resp[n,k] / w[b,k]
//   backward, with lambda[n] = glogpdf[n] / P and G[n,c,p] = gZ[n,c,p] - lambda[n] sum_k resp[n,k] d[n,k,c,p] / std[b,2k+c,p]:
//             gmean[b,2k+c,p]    = sum_s (lambda[n] resp[n,k] d / std + [z == k] G[n,c,p])
//             glog_std[b,2k+c,p] = sum_s (lambda[n] resp[n,k] (d^2 - 1) + [z == k] G[n,c,p] std[b,2k+c,p] eps[n,c,p])
// Sampler: a workgroup owns CHUNK consecutive pixels of one sample n; the sample is formed in fp32 (exp, one product, one
// sum: -ffp-contract=off), every term of A in float64 from there on (the difference flow - mean_k is exact in float64, 1 / std
// is the fp32 expf(-log_std)), summed per lane, then over the workgroup in the order of af_block_sum_f64 (common.hpp): one
// float64 partial per (n, chunk, k) in the work buffer.  A second, small launch adds the partials in chunk order and forms
// logpdf, resp and q in float64, rounded once.  A is a sum of 2 P terms of order one and resp a softmax of differences of such
// sums: nothing across lanes or chunks is fp32.
// Backward: a gather, one thread per pixel of item b, loops over s and k; it recomputes the sample from eps with the
// sampler's own fp32 expression (the same bits), does the rest in float64 and rounds every gradient element once.
// No atomics anywhere: the same code and the same bits in normal and deterministic mode.  Every element of every output is
// stored.
#include "common.hpp"

namespace {

constexpr int KMAX = 4;
constexpr int NT = 256;            // threads of a workgroup (4 waves)
constexpr int PIX = 4;             // pixels of a thread in the sampler: one float4 group, or 4 strided pixels
constexpr int CHUNK = NT * PIX;    // 1024 pixels per sampler workgroup

__device__ __forceinline__ float f4_at(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

__device__ __forceinline__ int comp_of(const long* __restrict__ comp, long i, int K) {
  const long z = comp[i];
  return z < 0 ? 0 : z >= K ? K - 1 : (int)z;  // a value outside 0..K-1 must not turn into an address
}

// The sample of one pixel and flow component from the drawn component's mean and log-std (the callers load them by z from
// memory, next to the 2K planes they hold in registers: a register array indexed by z would live in scratch).  fp32, one
// expression for the sampler, the backward and the entropy map.
__device__ __forceinline__ float mix_sample(float m, float l, float e) {
  const float t = expf(l) * e;
  return m + t;
}

// x[k] = -sum_c (log_std + d^2 / 2) of one pixel, in float64
__device__ __forceinline__ void mix_exponents(const float (&mu)[2 * KMAX], const float (&ls)[2 * KMAX], int K, float f0, float f1,
                                              double (&x)[KMAX]) {
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    x[k] = 0.;
    if (k < K) {
      const double d0 = ((double)f0 - (double)mu[2 * k]) * (double)expf(-ls[2 * k]);
      const double d1 = ((double)f1 - (double)mu[2 * k + 1]) * (double)expf(-ls[2 * k + 1]);
      x[k] = -(((double)ls[2 * k] + (double)ls[2 * k + 1]) + 0.5 * (d0 * d0 + d1 * d1));
    }
  }
}

// grid (chunks, S B).  VEC: float4 groups (P % 4 == 0 and every plane of every tensor 16-byte aligned, host-checked).
template <bool VEC>
__global__ __launch_bounds__(NT) void mixture_sample_kernel(const float* __restrict__ mean, long mean_bs,
                                                            const float* __restrict__ log_std, long ls_bs,
                                                            const float* __restrict__ eps, long eps_bs,
                                                            const long* __restrict__ comp, float* __restrict__ flow,
                                                            long flow_bs, double* __restrict__ work, int B, int S, int K,
                                                            long plane) {
  __shared__ double part[KMAX * (NT / AF_WAVE)];
  const int n = blockIdx.y, s = n / B, b = n % B;
  const int z = comp_of(comp, (long)b * S + s, K);
  const float* mb = mean + b * mean_bs;
  const float* lb = log_std + b * ls_bs;
  const float* eb = eps + n * eps_bs;
  float* fb = flow + n * flow_bs;
  const long base = (long)blockIdx.x * CHUNK;
  double acc[KMAX] = {0., 0., 0., 0.};
  if (VEC) {
    const long p = base + PIX * threadIdx.x;
    if (p < plane) {  // plane % 4 == 0: a group is inside or outside
      float4 mu4[2 * KMAX], ls4[2 * KMAX];
#pragma unroll
      for (int c = 0; c < 2 * KMAX; ++c)
        if (c < 2 * K) {
          mu4[c] = *reinterpret_cast<const float4*>(mb + c * plane + p);
          ls4[c] = *reinterpret_cast<const float4*>(lb + c * plane + p);
        }
      const float4 e0 = *reinterpret_cast<const float4*>(eb + p), e1 = *reinterpret_cast<const float4*>(eb + plane + p);
      const float4 mz0 = *reinterpret_cast<const float4*>(mb + 2 * z * plane + p);
      const float4 mz1 = *reinterpret_cast<const float4*>(mb + (2 * z + 1) * plane + p);
      const float4 lz0 = *reinterpret_cast<const float4*>(lb + 2 * z * plane + p);
      const float4 lz1 = *reinterpret_cast<const float4*>(lb + (2 * z + 1) * plane + p);
      float o0[PIX], o1[PIX];
#pragma unroll
      for (int j = 0; j < PIX; ++j) {
        float mu[2 * KMAX], ls[2 * KMAX];
#pragma unroll
        for (int c = 0; c < 2 * KMAX; ++c) {
          mu[c] = c < 2 * K ? f4_at(mu4[c], j) : 0.f;
          ls[c] = c < 2 * K ? f4_at(ls4[c], j) : 0.f;
        }
        o0[j] = mix_sample(f4_at(mz0, j), f4_at(lz0, j), f4_at(e0, j));
        o1[j] = mix_sample(f4_at(mz1, j), f4_at(lz1, j), f4_at(e1, j));
        double x[KMAX];
        mix_exponents(mu, ls, K, o0[j], o1[j], x);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[k] += x[k];
      }
      *reinterpret_cast<float4*>(fb + p) = make_float4(o0[0], o0[1], o0[2], o0[3]);
      *reinterpret_cast<float4*>(fb + plane + p) = make_float4(o1[0], o1[1], o1[2], o1[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const long p = base + threadIdx.x + (long)NT * j;
      if (p < plane) {
        float mu[2 * KMAX], ls[2 * KMAX];
#pragma unroll
        for (int c = 0; c < 2 * KMAX; ++c) {
          mu[c] = c < 2 * K ? mb[c * plane + p] : 0.f;
          ls[c] = c < 2 * K ? lb[c * plane + p] : 0.f;
        }
        const float f0 = mix_sample(mb[2 * z * plane + p], lb[2 * z * plane + p], eb[p]);
        const float f1 = mix_sample(mb[(2 * z + 1) * plane + p], lb[(2 * z + 1) * plane + p], eb[plane + p]);
        fb[p] = f0;
        fb[plane + p] = f1;
        double x[KMAX];
        mix_exponents(mu, ls, K, f0, f1, x);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[k] += x[k];
      }
    }
  }
  af_block_sum_f64<KMAX, NT>(acc, part);
  if (threadIdx.x == 0) {
    double* row = work + ((long)n * gridDim.x + blockIdx.x) * K;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) row[k] = acc[k];
  }
}

// grid (ceil(S B / 64)), one thread per sample n
__global__ __launch_bounds__(AF_WAVE) void mixture_logpdf_kernel(const double* __restrict__ work, int chunks,
                                                                 const float* __restrict__ weights,
                                                                 float* __restrict__ logpdf, float* __restrict__ resp,
                                                                 float* __restrict__ q, int B, long SB, int K, double inv_plane) {
  const long n = (long)blockIdx.x * AF_WAVE + threadIdx.x;
  if (n >= SB) return;
  const int b = (int)(n % B);
  double A[KMAX], e[KMAX], w[KMAX];
  double top = 0.;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    A[k] = 0.;
    w[k] = 0.;
    if (k < K) {
      double t = 0.;
      for (int c = 0; c < chunks; ++c) t += work[(n * chunks + c) * K + k];  // in chunk order
      A[k] = t;
      w[k] = (double)weights[(long)b * K + k];
      top = k == 0 ? t : (t > top ? t : top);
    }
  }
  double sum = 0.;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    e[k] = k < K ? exp(A[k] - top) : 0.;  // <= 1
    sum += w[k] * e[k];
  }
  logpdf[n] = (float)((top + log(sum)) * inv_plane);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      resp[n * K + k] = w[k] > 0. ? (float)(w[k] * e[k] / sum) : 0.f;
      q[n * K + k] = (float)(e[k] / sum);
    }
}

// grid (ceil(P / NT), B).  glogpdf NULL: no density term (resp is then not read); gZ NULL: no gradient into the samples.
__global__ __launch_bounds__(NT) void mixture_bwd_kernel(const float* __restrict__ mean, long mean_bs,
                                                         const float* __restrict__ log_std, long ls_bs,
                                                         const float* __restrict__ eps, long eps_bs,
                                                         const long* __restrict__ comp, const float* __restrict__ resp,
                                                         const float* __restrict__ glogpdf, const float* __restrict__ gZ,
                                                         long gz_bs, float* __restrict__ gmean, long gmean_bs,
                                                         float* __restrict__ gls, long gls_bs, int B, int S, int K, long plane) {
  const long p = (long)blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y;
  float mu[2 * KMAX], ls[2 * KMAX];
  double inv[2 * KMAX], gm[2 * KMAX], gl[2 * KMAX];
#pragma unroll
  for (int c = 0; c < 2 * KMAX; ++c) {
    mu[c] = c < 2 * K ? mean[b * mean_bs + c * plane + p] : 0.f;
    ls[c] = c < 2 * K ? log_std[b * ls_bs + c * plane + p] : 0.f;
    inv[c] = (double)expf(-ls[c]);
    gm[c] = 0.;
    gl[c] = 0.;
  }
  const double inv_plane = 1. / (double)plane;
  for (int s = 0; s < S; ++s) {
    const long n = (long)s * B + b;
    const int z = comp_of(comp, (long)b * S + s, K);
    const float e0 = eps[n * eps_bs + p], e1 = eps[n * eps_bs + plane + p];
    const float lz0 = log_std[b * ls_bs + 2 * z * plane + p], lz1 = log_std[b * ls_bs + (2 * z + 1) * plane + p];
    const float f0 = mix_sample(mean[b * mean_bs + 2 * z * plane + p], lz0, e0);
    const float f1 = mix_sample(mean[b * mean_bs + (2 * z + 1) * plane + p], lz1, e1);
    const double lam = glogpdf ? (double)glogpdf[n] * inv_plane : 0.;
    double G0 = gZ ? (double)gZ[n * gz_bs + p] : 0., G1 = gZ ? (double)gZ[n * gz_bs + plane + p] : 0.;
    if (glogpdf) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          const double lr = lam * (double)resp[n * K + k];
          const double d0 = ((double)f0 - (double)mu[2 * k]) * inv[2 * k];
          const double d1 = ((double)f1 - (double)mu[2 * k + 1]) * inv[2 * k + 1];
          const double a0 = lr * d0 * inv[2 * k], a1 = lr * d1 * inv[2 * k + 1];
          gm[2 * k] += a0;
          gm[2 * k + 1] += a1;
          gl[2 * k] += lr * (d0 * d0 - 1.);
          gl[2 * k + 1] += lr * (d1 * d1 - 1.);
          G0 -= a0;
          G1 -= a1;
        }
    }
    // the route through the sample: into the mean and the log-std of the component it was drawn from
    const double t0 = G0 * ((double)expf(lz0) * (double)e0), t1 = G1 * ((double)expf(lz1) * (double)e1);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K && z == k) {
        gm[2 * k] += G0;
        gm[2 * k + 1] += G1;
        gl[2 * k] += t0;
        gl[2 * k + 1] += t1;
      }
  }
#pragma unroll
  for (int c = 0; c < 2 * KMAX; ++c)
    if (c < 2 * K) {
      gmean[b * gmean_bs + c * plane + p] = (float)gm[c];
      gls[b * gls_bs + c * plane + p] = (float)gl[c];
    }
}

// grid (ceil(P / NT), B): out[b,p] = -(1 / n) sum_i (max_k x_k + log sum_k w_k exp(x_k - max)) over the n draws of the pixel
__global__ __launch_bounds__(NT) void mixture_entropy_kernel(const float* __restrict__ mean, long mean_bs,
                                                             const float* __restrict__ log_std, long ls_bs,
                                                             const float* __restrict__ weights, const long* __restrict__ comp,
                                                             const float* __restrict__ eps, long eps_bs,
                                                             float* __restrict__ out, int B, int n, int K, long plane) {
  const long p = (long)blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y;
  float mu[2 * KMAX], ls[2 * KMAX];
  double w[KMAX];
#pragma unroll
  for (int c = 0; c < 2 * KMAX; ++c) {
    mu[c] = c < 2 * K ? mean[b * mean_bs + c * plane + p] : 0.f;
    ls[c] = c < 2 * K ? log_std[b * ls_bs + c * plane + p] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) w[k] = k < K ? (double)weights[(long)b * K + k] : 0.;
  double acc = 0.;
  for (int i = 0; i < n; ++i) {
    const long row = (long)i * B + b;
    const int z = comp_of(comp, (long)b * n + i, K);
    const float f0 = mix_sample(mean[b * mean_bs + 2 * z * plane + p], log_std[b * ls_bs + 2 * z * plane + p], eps[row * eps_bs + p]);
    const float f1 = mix_sample(mean[b * mean_bs + (2 * z + 1) * plane + p], log_std[b * ls_bs + (2 * z + 1) * plane + p],
                                eps[row * eps_bs + plane + p]);
    double x[KMAX];
    mix_exponents(mu, ls, K, f0, f1, x);
    double top = x[0];
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
      if (k < K && x[k] > top) top = x[k];
    double sum = 0.;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) sum += w[k] * exp(x[k] - top);
    acc -= top + log(sum);
  }
  out[(long)b * plane + p] = (float)(acc / (double)n);
}

inline int check_dims(int B, int S, int K, int M, int N) {
  AF_REQUIRE(K >= 1 && K <= KMAX, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && S >= 1 && M >= 1 && N >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE((long)M * N <= 0x7fffffffL && (long)S * B <= 65535, ARFLOW_ESHAPE);  // gridDim.y of the sampler
  return ARFLOW_OK;
}

}  // namespace

extern "C" long arflow_mixture_work_size(int B, int S, int K, int M, int N) {
  const int rc = check_dims(B, S, K, M, N);
  if (rc != ARFLOW_OK) return rc;
  return (long)S * B * af_cdiv((long)M * N, CHUNK) * K;
}

extern "C" int arflow_mixture_sample_fwd(const float* mean, long mean_bs, const float* log_std, long ls_bs, const float* eps,
                                         long eps_bs, const long* comp, float* flow, long flow_bs, double* work, int B, int S,
                                         int K, int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(mean);
  AF_REQUIRE_PTR(log_std);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(comp);
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(work);
  const int rc = check_dims(B, S, K, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N, SB = (long)S * B;
  AF_REQUIRE(af_stride_ok(mean_bs, B, 2L * K * plane) && af_stride_ok(ls_bs, B, 2L * K * plane) &&
                 af_stride_ok(eps_bs, SB, 2 * plane) && af_stride_ok(flow_bs, SB, 2 * plane),
             ARFLOW_ESHAPE);
  const bool vec = plane % 4 == 0 && af_vec4_ok(mean, mean_bs, B) && af_vec4_ok(log_std, ls_bs, B) &&
                   af_vec4_ok(eps, eps_bs, SB) && af_vec4_ok(flow, flow_bs, SB);
  const dim3 grid(af_cdiv(plane, CHUNK), (unsigned)SB);
  if (vec)
    hipLaunchKernelGGL(mixture_sample_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, mean, mean_bs, log_std, ls_bs, eps,
                       eps_bs, comp, flow, flow_bs, work, B, S, K, plane);
  else
    hipLaunchKernelGGL(mixture_sample_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, mean, mean_bs, log_std, ls_bs, eps,
                       eps_bs, comp, flow, flow_bs, work, B, S, K, plane);
  return af_launch_status();
}

extern "C" int arflow_mixture_logpdf_fwd(const double* work, const float* weights, float* logpdf, float* resp, float* q, int B,
                                         int S, int K, int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(work);
  AF_REQUIRE_PTR(weights);
  AF_REQUIRE_PTR(logpdf);
  AF_REQUIRE_PTR(resp);
  AF_REQUIRE_PTR(q);
  const int rc = check_dims(B, S, K, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N, SB = (long)S * B;
  hipLaunchKernelGGL(mixture_logpdf_kernel, dim3(af_cdiv(SB, AF_WAVE)), dim3(AF_WAVE), 0, (hipStream_t)stream, work,
                     af_cdiv(plane, CHUNK), weights, logpdf, resp, q, B, SB, K, 1. / (double)plane);
  return af_launch_status();
}

extern "C" int arflow_mixture_bwd(const float* mean, long mean_bs, const float* log_std, long ls_bs, const float* eps,
                                  long eps_bs, const long* comp, const float* resp, const float* glogpdf, const float* gZ,
                                  long gz_bs, float* gmean, long gmean_bs, float* glog_std, long gls_bs, int B, int S, int K,
                                  int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(mean);
  AF_REQUIRE_PTR(log_std);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(comp);
  AF_REQUIRE_PTR(gmean);
  AF_REQUIRE_PTR(glog_std);
  if (glogpdf) AF_REQUIRE_PTR(resp);
  const int rc = check_dims(B, S, K, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N, SB = (long)S * B;
  AF_REQUIRE(af_stride_ok(mean_bs, B, 2L * K * plane) && af_stride_ok(ls_bs, B, 2L * K * plane) &&
                 af_stride_ok(eps_bs, SB, 2 * plane) && (!gZ || af_stride_ok(gz_bs, SB, 2 * plane)) &&
                 af_stride_ok(gmean_bs, B, 2L * K * plane) && af_stride_ok(gls_bs, B, 2L * K * plane),
             ARFLOW_ESHAPE);
  hipLaunchKernelGGL(mixture_bwd_kernel, dim3(af_cdiv(plane, NT), B), dim3(NT), 0, (hipStream_t)stream, mean, mean_bs, log_std,
                     ls_bs, eps, eps_bs, comp, resp, glogpdf, gZ, gz_bs, gmean, gmean_bs, glog_std, gls_bs, B, S, K, plane);
  return af_launch_status();
}

extern "C" int arflow_mixture_entropy_map(const float* mean, long mean_bs, const float* log_std, long ls_bs,
                                          const float* weights, const long* comp, const float* eps, long eps_bs, float* out,
                                          int B, int n, int K, int M, int N, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(mean);
  AF_REQUIRE_PTR(log_std);
  AF_REQUIRE_PTR(weights);
  AF_REQUIRE_PTR(comp);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(out);
  const int rc = check_dims(B, n, K, M, N);
  if (rc != ARFLOW_OK) return rc;
  const long plane = (long)M * N;
  AF_REQUIRE(af_stride_ok(mean_bs, B, 2L * K * plane) && af_stride_ok(ls_bs, B, 2L * K * plane) &&
                 af_stride_ok(eps_bs, (long)n * B, 2 * plane),
             ARFLOW_ESHAPE);
  hipLaunchKernelGGL(mixture_entropy_kernel, dim3(af_cdiv(plane, NT), B), dim3(NT), 0, (hipStream_t)stream, mean, mean_bs,
                     log_std, ls_bs, weights, comp, eps, eps_bs, out, B, n, K, plane);
  return af_launch_status();
}
