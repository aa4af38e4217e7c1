// One-pass EM statistics of the Gaussian-mixture penalty fit, and the elementwise log-density of the fitted mixture
// (DESIGN.md section 44).
//   train_penalty_em.py:86-220 (class EM), losses/uflow_elbo_loss.py:99-105 (log_gmm).
// The reference's update_xi materialises the m x k responsibility matrix xi; every later quantity of EM.update is a function
// of four k-vectors of sums over the samples, so arflow_em_stats forms xi of one sample in registers and keeps the sums only.
//
// E-STEP, float64 throughout.  The caller passes  logw_j = digamma(alpha_bar_j) - digamma(sum alpha_bar) + log(beta_j) / 2  (the
// sqrt(beta) factor of update_xi inside the exponent).  Per sample x (fp32 samples are widened first) with weight w (1 without
// x1), every operation rounded once (-ffp-contract=off), j ascending:
//     d_j = x - mu_j       q_j = d_j d_j       a_j = (-beta_j) q_j / 2 + logw_j       c = max_j a_j
//     e_j = exp(a_j - c)   den = ((e_0 + e_1) + ...) + e_{k-1}       L = log(den)
//     xi_j = e_j / den     lxi_j = (a_j - c) - L        (ONE log per sample; finite where xi_j underflows, so xi_j lxi_j = -0)
//     (only e_j is kept between the passes over j; d_j, q_j and a_j - c are formed again by the same operations)
//     t_j = w xi_j         S0_j += t_j      S1_j += t_j x      S2_j += t_j q_j      H_j += t_j lxi_j
// SUMS.  Workgroup b owns samples [b per, (b + 1) per), per = em_share(m); lane t adds samples lo + t, lo + t + 256, ... in that
// order, the workgroup adds its lanes by af_block_sum_f64 (common.hpp) and STORES 4 k doubles into part[b][4][k] (S0, S1, S2,
// H).  No atomics, no zero-fill: two calls give the same bits in either mode.  arflow_em_fold adds the partials of every column
// in index order to 0.0.
// The mixture parameters (logw, -beta, mu) are staged once per workgroup in LDS: as per-lane arrays behind uniform addresses they
// took 96 scalar registers at K = 16 and spilled.  Two instantiations, K <= 8 (two waves per SIMD) and K <= 16 (one); the terms
// of j >= k are skipped by a wave-uniform branch (register counts and the measured consequence: DESIGN.md section 44).
//
// LOG_GMM, in the dtype T of x (fp32 or fp64), the reference's order:  w_j = pi_j sqrt(beta_j) / sqrt(2 pi) arrives as float64
// and is rounded to T once, as beta_j is:
//     s = x x     arg_j = (-beta_j) s / 2     c = max_j arg_j     p_j = w_j exp(arg_j - c)     den = ((p_0 + p_1) + ...)
//     out = c + log(den)                      backward: gx = gout * -(((p_0 beta_0 + p_1 beta_1) + ...) / den) x
#include "common.hpp"

#include <cmath>

namespace {

constexpr int EM_NT = 256;
constexpr long EM_UNIT = ARFLOW_EM_UNIT;  // a workgroup's share is a multiple of this
constexpr int EM_MAX_PARTS = ARFLOW_EM_MAX_PARTS;
constexpr int EM_KMAX = ARFLOW_EM_KMAX;

inline long em_share(long m) {
  const long units = (m + EM_UNIT - 1) / EM_UNIT;
  return EM_UNIT * ((units + EM_MAX_PARTS - 1) / EM_MAX_PARTS);
}
inline int em_partials(long m) {
  const long per = em_share(m);
  return (int)((m + per - 1) / per);
}

template <typename T, int KT>
__global__ __launch_bounds__(EM_NT, KT <= 8 ? 2 : 1) void em_stats_kernel(const T* __restrict__ x0, const T* __restrict__ x1,
                                                          const double* __restrict__ logw, const double* __restrict__ beta,
                                                          const double* __restrict__ mu, double* __restrict__ part, long m,
                                                          long per, int k) {
  __shared__ double scratch[4 * KT * (EM_NT / AF_WAVE)];
  __shared__ double lw[KT], nb[KT], mj[KT];
  if ((int)threadIdx.x < k) lw[threadIdx.x] = logw[threadIdx.x], nb[threadIdx.x] = -beta[threadIdx.x], mj[threadIdx.x] = mu[threadIdx.x];
  __syncthreads();
  double acc[4 * KT];
#pragma unroll
  for (int j = 0; j < 4 * KT; ++j) acc[j] = 0.0;
  const long lo = (long)blockIdx.x * per, hi = min(lo + per, m);
#pragma unroll 1
  for (long i = lo + threadIdx.x; i < hi; i += EM_NT) {
    const double x = (double)x0[i];
    const double w = x1 != nullptr ? (double)x1[i] : 1.0;
    // only e_j is kept between the three passes over j: d_j, q_j and a_j are formed again by the same operations (the same bits)
    double e[KT];
    double c = 0.0;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      if (j < k) {
        const double d = x - mj[j];
        const double a = nb[j] * (d * d) / 2.0 + lw[j];
        c = j == 0 ? a : fmax(c, a);
      }
    }
    double den = 0.0;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      if (j < k) {
        const double d = x - mj[j];
        e[j] = exp((nb[j] * (d * d) / 2.0 + lw[j]) - c);
        den = j == 0 ? e[0] : den + e[j];
      }
    }
    const double L = log(den);
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      if (j < k) {
        const double d = x - mj[j];
        const double q = d * d;
        const double t = w * (e[j] / den);
        acc[j] += t;
        acc[KT + j] += t * x;
        acc[2 * KT + j] += t * q;
        acc[3 * KT + j] += t * (((nb[j] * q / 2.0 + lw[j]) - c) - L);
      }
    }
  }
  af_block_sum_f64<4 * KT, EM_NT>(acc, scratch);
  if (threadIdx.x == 0) {
    double* __restrict__ o = part + (long)blockIdx.x * 4 * k;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < KT; ++j)
        if (j < k) o[s * k + j] = acc[s * KT + j];
  }
}

// one lane per column of part[nparts][ncols]: the partials in index order, added to 0.0
__global__ __launch_bounds__(64) void em_fold_kernel(const double* __restrict__ part, double* __restrict__ stats, int nparts,
                                                     int ncols) {
  const int c = threadIdx.x;
  if (c >= ncols) return;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(long)b * ncols + c];
  stats[c] = s;
}

constexpr int LG_NT = 256;

template <typename T>
struct LgParams {
  T w[EM_KMAX], nb[EM_KMAX];
};

template <typename T>
__device__ __forceinline__ void lg_load(const double* __restrict__ w, const double* __restrict__ beta, int k, LgParams<T>& p) {
#pragma unroll
  for (int j = 0; j < EM_KMAX; ++j) {
    const int jj = j < k ? j : 0;
    p.w[j] = (T)w[jj], p.nb[j] = -(T)beta[jj];
  }
}

// den and (BWD) the beta-weighted numerator of one element; returns c
template <typename T, bool BWD>
__device__ __forceinline__ T lg_element(const LgParams<T>& p, int k, T x, T& den, T& num) {
  const T s = x * x;
  T arg[EM_KMAX];
  T c = (T)0;
#pragma unroll
  for (int j = 0; j < EM_KMAX; ++j) {
    if (j < k) {
      arg[j] = p.nb[j] * s / (T)2;
      c = j == 0 ? arg[0] : (arg[j] > c ? arg[j] : c);
    }
  }
  den = (T)0, num = (T)0;
#pragma unroll
  for (int j = 0; j < EM_KMAX; ++j) {
    if (j < k) {
      const T e = p.w[j] * (T)exp(arg[j] - c);  // exp of a T: expf for fp32
      den = j == 0 ? e : den + e;
      if (BWD) {
        const T b = e * -p.nb[j];
        num = j == 0 ? b : num + b;
      }
    }
  }
  return c;
}

template <typename T>
__global__ __launch_bounds__(LG_NT) void log_gmm_fwd_kernel(const T* __restrict__ x, const double* __restrict__ w,
                                                             const double* __restrict__ beta, T* __restrict__ out, long n, int k) {
  LgParams<T> p;
  lg_load(w, beta, k, p);
  for (long i = (long)blockIdx.x * LG_NT + threadIdx.x; i < n; i += (long)gridDim.x * LG_NT) {
    T den, num;
    const T c = lg_element<T, false>(p, k, x[i], den, num);
    out[i] = c + (T)log(den);
  }
}

template <typename T>
__global__ __launch_bounds__(LG_NT) void log_gmm_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gout,
                                                             const double* __restrict__ w, const double* __restrict__ beta,
                                                             T* __restrict__ gx, long n, int k) {
  LgParams<T> p;
  lg_load(w, beta, k, p);
  for (long i = (long)blockIdx.x * LG_NT + threadIdx.x; i < n; i += (long)gridDim.x * LG_NT) {
    T den, num;
    const T xv = x[i];
    lg_element<T, true>(p, k, xv, den, num);
    gx[i] = gout[i] * (-(num / den) * xv);
  }
}

inline bool em_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned lg_grid(long n) {
  const long nb = (n + LG_NT - 1) / LG_NT;
  return (unsigned)(nb < 4096 ? nb : 4096);
}

}  // namespace

extern "C" int arflow_em_partials(long m) {
  AF_REQUIRE(m >= 1, ARFLOW_ESHAPE);
  return em_partials(m);
}

extern "C" int arflow_em_stats(const void* x0, const void* x1, long m, int is_f64, const double* logw, const double* beta,
                               const double* mu, int k, double* part, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x0);
  AF_REQUIRE_PTR(logw);
  AF_REQUIRE_PTR(beta);
  AF_REQUIRE_PTR(mu);
  AF_REQUIRE_PTR(part);
  AF_REQUIRE(m >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(k >= 1 && k <= EM_KMAX && (is_f64 == 0 || is_f64 == 1), ARFLOW_EPARAM);
  const size_t a = is_f64 ? 8 : 4;
  AF_REQUIRE(em_aligned(x0, a) && em_aligned(x1, a) && em_aligned(logw, 8) && em_aligned(beta, 8) && em_aligned(mu, 8) &&
                 em_aligned(part, 8),
             ARFLOW_EPARAM);
  const long per = em_share(m);
  const dim3 grid((unsigned)em_partials(m)), block(EM_NT);
  const hipStream_t s = (hipStream_t)stream;
#define EM_LAUNCH(T, KT) \
  hipLaunchKernelGGL((em_stats_kernel<T, KT>), grid, block, 0, s, (const T*)x0, (const T*)x1, logw, beta, mu, part, m, per, k)
  if (is_f64) {
    if (k <= 8)
      EM_LAUNCH(double, 8);
    else
      EM_LAUNCH(double, 16);
  } else {
    if (k <= 8)
      EM_LAUNCH(float, 8);
    else
      EM_LAUNCH(float, 16);
  }
#undef EM_LAUNCH
  return af_launch_status();
}

extern "C" int arflow_em_fold(const double* part, int nparts, int k, double* stats, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(part);
  AF_REQUIRE_PTR(stats);
  AF_REQUIRE(nparts >= 1 && nparts <= EM_MAX_PARTS, ARFLOW_ESHAPE);
  AF_REQUIRE(k >= 1 && k <= EM_KMAX, ARFLOW_EPARAM);
  AF_REQUIRE(em_aligned(part, 8) && em_aligned(stats, 8), ARFLOW_EPARAM);
  hipLaunchKernelGGL(em_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, stats, nparts, 4 * k);
  return af_launch_status();
}

extern "C" int arflow_log_gmm_fwd(const void* x, long n, int is_f64, const double* w, const double* beta, int k, void* out,
                                  arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(w);
  AF_REQUIRE_PTR(beta);
  AF_REQUIRE_PTR(out);
  AF_REQUIRE(n >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(k >= 1 && k <= EM_KMAX && (is_f64 == 0 || is_f64 == 1), ARFLOW_EPARAM);
  const size_t a = is_f64 ? 8 : 4;
  AF_REQUIRE(em_aligned(x, a) && em_aligned(out, a) && em_aligned(w, 8) && em_aligned(beta, 8), ARFLOW_EPARAM);
  const dim3 grid(lg_grid(n)), block(LG_NT);
  if (is_f64)
    hipLaunchKernelGGL(log_gmm_fwd_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, w, beta, (double*)out, n, k);
  else
    hipLaunchKernelGGL(log_gmm_fwd_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, w, beta, (float*)out, n, k);
  return af_launch_status();
}

extern "C" int arflow_log_gmm_bwd(const void* x, const void* gout, long n, int is_f64, const double* w, const double* beta,
                                  int k, void* gx, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(gout);
  AF_REQUIRE_PTR(w);
  AF_REQUIRE_PTR(beta);
  AF_REQUIRE_PTR(gx);
  AF_REQUIRE(n >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(k >= 1 && k <= EM_KMAX && (is_f64 == 0 || is_f64 == 1), ARFLOW_EPARAM);
  const size_t a = is_f64 ? 8 : 4;
  AF_REQUIRE(em_aligned(x, a) && em_aligned(gout, a) && em_aligned(gx, a) && em_aligned(w, 8) && em_aligned(beta, 8),
             ARFLOW_EPARAM);
  const dim3 grid(lg_grid(n)), block(LG_NT);
  if (is_f64)
    hipLaunchKernelGGL(log_gmm_bwd_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, (const double*)gout, w, beta,
                       (double*)gx, n, k);
  else
    hipLaunchKernelGGL(log_gmm_bwd_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, (const float*)gout, w, beta,
                       (float*)gx, n, k);
  return af_launch_status();
}
