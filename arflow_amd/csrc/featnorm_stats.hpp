// The arithmetic of `normalize_features` (models/pwclite_uflow.py:30-38 'joint', models/uflow_model.py:8-50 as PWCFlow
// calls it 'avg'), stated once: device functions, no kernels.  featnorm.hip (the stand-alone op) and the level kernels
// that fold the normalisation into the warp / correlation launches (warp.hip, corr_v2.hpp, level_small.hip) are loop
// skeletons and calls of these.  tests/corr_ref.py derives its float64 bounds from what is written HERE: VPT values per
// fp32 partial, double from there on, Q centred on the rounded mu, three backward coefficients rounded to fp32.
// Built with -ffp-contract=off: every operation order below is part of the contract (outputs are pinned bit for bit).
//
// Partial sums travel as rows of 4 doubles (sum x1, sum x1^2, sum x2, sum x2^2): every workgroup of a reduction
// pass STORES its row ([B][rows][4]); a consumer adds a sample's rows (one row per lane, wave-reduced) -- no
// zero-fill, no atomics, a fixed summation order.
#pragma once
#include "common.hpp"

namespace featnorm {

// ---- moments: fp32 steps, partial sums of a thread, totals -> statistics ----

// one float4 / one value into a running fp32 (sum, sum of squares)
__device__ __forceinline__ void moment_step(const float4& u, float& s, float& q) {
  s += (u.x + u.y) + (u.z + u.w);
  q = fmaf(u.x, u.x, fmaf(u.y, u.y, fmaf(u.z, u.z, fmaf(u.w, u.w, q))));
}
__device__ __forceinline__ void moment_step(float v, float& s, float& q) { s += v, q = fmaf(v, v, q); }

constexpr int VPT = 16;  // floats per thread, tensor and trip of the float4 loops (4 float4): the longest fp32 partial

// A thread's share of (sum x1, sum x1^2, sum x2, sum x2^2) over the n values at p1, p2, as block `blk` of `nblk` blocks
// of NTH threads: fp32 over at most VPT values per tensor, double beyond; the scalar tail (all of it when n % 4 != 0:
// rows are 16-byte aligned only when n % 4 == 0) is double from the first value.
template <int NTH>
__device__ __forceinline__ void moment_partials(const float* __restrict__ p1, const float* __restrict__ p2, long n, long blk,
                                                long nblk, double (&s)[4]) {
  s[0] = s[1] = s[2] = s[3] = 0.0;
  const long n4 = (n % 4 == 0) ? n / 4 : 0;
  for (long i0 = blk * NTH * (VPT / 4); i0 < n4; i0 += nblk * NTH * (VPT / 4)) {
    float a1 = 0.f, q1 = 0.f, a2 = 0.f, q2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPT / 4; ++k) {
      const long i = i0 + (long)k * NTH + threadIdx.x;
      if (i < n4) {
        moment_step(reinterpret_cast<const float4*>(p1)[i], a1, q1);
        moment_step(reinterpret_cast<const float4*>(p2)[i], a2, q2);
      }
    }
    s[0] += (double)a1, s[1] += (double)q1, s[2] += (double)a2, s[3] += (double)q2;
  }
  for (long i = 4 * n4 + blk * NTH + threadIdx.x; i < n; i += nblk * NTH) {
    const float u = p1[i], v = p2[i];
    s[0] += (double)u, s[1] += (double)u * (double)u, s[2] += (double)v, s[3] += (double)v * (double)v;
  }
}

struct Moments {
  float m1, m2, mu, var;
};

// (sum x1, sum x1^2, sum x2, sum x2^2) over n values per tensor -> the sample's statistics
__device__ __forceinline__ Moments moments_from_totals(const double (&a)[4], long n, int mode) {
  const double dn = (double)n;
  const double m1 = a[0] / dn, m2 = a[2] / dn;
  double mu, var;
  if (mode == ARFLOW_FEATNORM_JOINT) {
    const double N = 2.0 * dn;
    mu = (a[0] + a[2]) / N;
    var = ((a[1] + a[3]) - N * mu * mu) / (N - 1.0);
  } else {
    mu = 0.5 * (m1 + m2);
    var = 0.5 * ((a[1] - dn * m1 * m1) + (a[3] - dn * m2 * m2)) / (dn - 1.0);
  }
  var = var > 0.0 ? var : 0.0;
  Moments m;
  m.m1 = (float)m1, m.m2 = (float)m2, m.mu = (float)mu, m.var = (float)var;
  return m;
}

// the standard deviation the outputs are divided by, and the row of `stats` the backward reads: (m1, m2, mu, sd)
__device__ __forceinline__ float sd_of(const Moments& m) { return sqrtf(m.var + 1e-16f); }
__device__ __forceinline__ void store_stats(float* __restrict__ st, const Moments& m, float sd) {
  st[0] = m.m1, st[1] = m.m2, st[2] = m.mu, st[3] = sd;
}

// sum of the first NV entries of `nrows` rows of 4 doubles: one row per lane, then a wave reduction (every lane gets it)
template <int NV>
__device__ __forceinline__ void sum_rows(const double* rows, int nrows, double (&a)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) a[k] = 0.0;
  for (int r = threadIdx.x & 63; r < nrows; r += 64) {
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] += rows[4 * r + k];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off, 64);
  }
}

__device__ __forceinline__ Moments moments_of(const double* rows, int nrows, long n, int mode) {
  double a[4];
  sum_rows<4>(rows, nrows, a);
  return moments_from_totals(a, n, mode);
}

// sum of `nrows` rows of 2 doubles (the rows arflow_bias_act_fwd_mom leaves): one row per lane + wave reduction
__device__ __forceinline__ void sum_rows2(const double* rows, int nrows, double& s, double& q) {
  s = 0.0, q = 0.0;
  for (int r = threadIdx.x & 63; r < nrows; r += 64) s += rows[2 * r], q += rows[2 * r + 1];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64), q += __shfl_xor(q, off, 64);
}

// The sample's statistics from up to three partial-moment sources: `acc` rows of 4 doubles (sum x1, sum x1^2, sum x2,
// sum x2^2; the warp launch / moment pass), and optional 2-column rows for the first (`r1`) and the second map (`r2`)
// taken in the conv epilogue that produced them (they REPLACE the corresponding columns of acc; acc may be null when both
// are given).
struct MomentSrc {
  const double* acc;
  int nrows;
  const double* r1;
  int n1;
  const double* r2;
  int n2;
};
__device__ __forceinline__ Moments moments_of(const MomentSrc& m, int b, long n, int mode) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (m.acc && m.nrows > 0) sum_rows<4>(m.acc + 4L * m.nrows * b, m.nrows, a);
  if (m.r1) sum_rows2(m.r1 + 2L * m.n1 * b, m.n1, a[0], a[1]);
  if (m.r2) sum_rows2(m.r2 + 2L * m.n2 * b, m.n2, a[2], a[3]);
  return moments_from_totals(a, n, mode);
}

// ---- forward apply: y_i = (x_i - mu) / sd, float4 part + scalar tail, elements first, first + stride, ... ----
__device__ __forceinline__ float4 normalized(const float4& u, float mu, float sd) {
  return make_float4((u.x - mu) / sd, (u.y - mu) / sd, (u.z - mu) / sd, (u.w - mu) / sd);
}
__device__ __forceinline__ void apply_fwd(const float* __restrict__ p1, const float* __restrict__ p2, float* __restrict__ o1,
                                          float* __restrict__ o2, long n, float mu, float sd, long first, long stride) {
  const long n4 = (n % 4 == 0) ? n / 4 : 0;
  for (long i = first; i < n4; i += stride) {
    const float4 u = reinterpret_cast<const float4*>(p1)[i];
    const float4 v = reinterpret_cast<const float4*>(p2)[i];
    reinterpret_cast<float4*>(o1)[i] = normalized(u, mu, sd);
    reinterpret_cast<float4*>(o2)[i] = normalized(v, mu, sd);
  }
  for (long i = 4 * n4 + first; i < n; i += stride) {
    o1[i] = (p1[i] - mu) / sd;
    o2[i] = (p2[i] - mu) / sd;
  }
}

// ---- backward.  With r = 1/sd, G = sum g, Q = sum g (x - mu) (both tensors):
//   JOINT: dx = r g - r G / N - r^3 Q (x - mu) / (N - 1),           N = 2n
//   AVG:   dx_i = r g - r G / (2n) - r^3 Q (x - m_i) / (2 (n - 1))

// gradient of y1 with its optional second part `b` (nullable) added on load
__device__ __forceinline__ float4 ld4_sum(const float* a, const float* b, long i) {
  float4 v = reinterpret_cast<const float4*>(a)[i];
  if (b) {
    const float4 w = reinterpret_cast<const float4*>(b)[i];
    v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
  }
  return v;
}
__device__ __forceinline__ float ld_sum(const float* a, const float* b, long i) { return a[i] + (b ? b[i] : 0.f); }

// A thread's share of (G, Q) over one sample (g1b nullable), blocks and precisions as moment_partials: one fp32 partial
// holds up to 2 VPT values, both tensors'.
template <int NTH>
__device__ __forceinline__ void bwd_partials(const float* __restrict__ g1, const float* __restrict__ g1b,
                                             const float* __restrict__ g2, const float* __restrict__ x1,
                                             const float* __restrict__ x2, float mu, long n, long blk, long nblk,
                                             double (&s)[2]) {
  s[0] = s[1] = 0.0;
  const long n4 = (n % 4 == 0) ? n / 4 : 0;
  for (long i0 = blk * NTH * (VPT / 4); i0 < n4; i0 += nblk * NTH * (VPT / 4)) {
    float sg = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < VPT / 4; ++k) {
      const long i = i0 + (long)k * NTH + threadIdx.x;
      if (i < n4) {
        const float4 ga = ld4_sum(g1, g1b, i), xa = reinterpret_cast<const float4*>(x1)[i];
        const float4 gb = reinterpret_cast<const float4*>(g2)[i], xb = reinterpret_cast<const float4*>(x2)[i];
        sg += ((ga.x + ga.y) + (ga.z + ga.w)) + ((gb.x + gb.y) + (gb.z + gb.w));
        sq = fmaf(ga.x, xa.x - mu, fmaf(ga.y, xa.y - mu, fmaf(ga.z, xa.z - mu, fmaf(ga.w, xa.w - mu, sq))));
        sq = fmaf(gb.x, xb.x - mu, fmaf(gb.y, xb.y - mu, fmaf(gb.z, xb.z - mu, fmaf(gb.w, xb.w - mu, sq))));
      }
    }
    s[0] += (double)sg, s[1] += (double)sq;
  }
  for (long i = 4 * n4 + blk * NTH + threadIdx.x; i < n; i += nblk * NTH) {
    const float ga = ld_sum(g1, g1b, i), gb = g2[i];
    s[0] += (double)ga + (double)gb;
    s[1] += (double)ga * (double)(x1[i] - mu) + (double)gb * (double)(x2[i] - mu);
  }
}

// the rule's three coefficients, rounded to fp32, and the centres of the two tensors (mu, or m1 / m2 in AVG mode)
struct NormBwd {
  float rf, cg, cq, c1, c2;
};
// st: the sample's row of `stats`; n: values per tensor
__device__ __forceinline__ NormBwd norm_bwd_coeffs(double G, double Q, const float* st, long n, int mode) {
  const double r = 1.0 / (double)st[3], dn = (double)n;
  NormBwd nb;
  nb.rf = (float)r;
  nb.cg = (float)(r * G / (2.0 * dn));
  nb.cq = (float)(mode == ARFLOW_FEATNORM_JOINT ? r * r * r * Q / (2.0 * dn - 1.0) : r * r * r * Q / (2.0 * (dn - 1.0)));
  nb.c1 = mode == ARFLOW_FEATNORM_JOINT ? st[2] : st[0];
  nb.c2 = mode == ARFLOW_FEATNORM_JOINT ? st[2] : st[1];
  return nb;
}
// (G, Q) as the sample's `nrows` rows of 4 doubles that a sum pass left (entries 0, 1)
__device__ __forceinline__ NormBwd norm_bwd_coeffs(const double* rows, int nrows, const float* st, long n, int mode) {
  double gq[2];
  sum_rows<2>(rows, nrows, gq);
  return norm_bwd_coeffs(gq[0], gq[1], st, n, mode);
}
// c: nb.c1 for the first tensor, nb.c2 for the second
__device__ __forceinline__ float norm_bwd_apply(const NormBwd& nb, float g, float x, float c) {
  return fmaf(nb.rf, g, -nb.cg) - nb.cq * (x - c);
}
__device__ __forceinline__ float4 norm_bwd_apply(const NormBwd& nb, const float4& g, const float4& x, float c) {
  return make_float4(norm_bwd_apply(nb, g.x, x.x, c), norm_bwd_apply(nb, g.y, x.y, c), norm_bwd_apply(nb, g.z, x.z, c),
                     norm_bwd_apply(nb, g.w, x.w, c));
}

// backward apply over one sample (d1, d2 nullable: that gradient is not asked for), elements as apply_fwd
__device__ __forceinline__ void apply_bwd(const NormBwd& nb, const float* __restrict__ g1, const float* __restrict__ g1b,
                                          const float* __restrict__ g2, const float* __restrict__ x1,
                                          const float* __restrict__ x2, float* __restrict__ d1, float* __restrict__ d2, long n,
                                          long first, long stride) {
  const long n4 = (n % 4 == 0) ? n / 4 : 0;
  for (long i = first; i < n4; i += stride) {
    if (d1) reinterpret_cast<float4*>(d1)[i] = norm_bwd_apply(nb, ld4_sum(g1, g1b, i), reinterpret_cast<const float4*>(x1)[i], nb.c1);
    if (d2)
      reinterpret_cast<float4*>(d2)[i] =
          norm_bwd_apply(nb, reinterpret_cast<const float4*>(g2)[i], reinterpret_cast<const float4*>(x2)[i], nb.c2);
  }
  for (long i = 4 * n4 + first; i < n; i += stride) {
    if (d1) d1[i] = norm_bwd_apply(nb, ld_sum(g1, g1b, i), x1[i], nb.c1);
    if (d2) d2[i] = norm_bwd_apply(nb, g2[i], x2[i], nb.c2);
  }
}

}  // namespace featnorm
