// The selectable penalties of UFlowElboLoss (losses/penalty_functions.py, losses/uflow_elbo_loss.py:99-105) on the device: ONE
// statement of every pair (rho, rho'), used by the penalised census forwards (census_pen.hip) and the penalised smoothness
// kernels (smooth_pen.hip).  DESIGN.md section 45.
//
//   kind          rho(x)                                      used as
//   IDENTITY      x
//   CHARBONNIER   sqrt(x + 1e-6)                              penalty_functions.py:6-7, eps = 0.001
//   ABS_ROBUST    (|x| + 0.01)^0.4                            penalty_functions.py:3-4
//   GMM           -log sum_j w_j exp(-beta_j x^2 / 2)         data term, x = soft census distance
//   GMM_SQ        -log sum_j w_j exp(-beta_j x   / 2)         smoothness, x = squared difference
//
// The kind is a compile-time policy of the kernels (one instantiation each); the mixture parameters travel BY VALUE in the
// kernel arguments (PenArgs, 132 bytes): every lane reads the same w_j / beta_j, so the compiler fetches them with scalar
// loads from the constant kernel-argument segment inside a ROLLED loop over j -- two SGPRs live per iteration instead of 32
// for a k = 16 array (the float64 EM kernel of penalty_em.hip spilled SGPRs with per-lane arrays behind uniform addresses), no
// LDS, no staging barrier.  Two passes over j: the maximum first, then the sums with arg_j recomputed (same bits), so no
// per-lane array exists either.  exp and log are the correctly-rounded-to-2-ulp library forms (expf, logf), not the
// v_exp / v_log approximations: <= 16 of them per pixel are nothing next to the 49-pair census, and the error bounds of
// tests/elbo_penalty_ref.py stay simple.  The powers of ABS_ROBUST use exp2f / __log2f exactly as ham_loss_terms does.
#pragma once
#include <cmath>

#include "common.hpp"

namespace {

struct PenArgs {
  int k;
  float w[ARFLOW_EM_KMAX];
  float beta[ARFLOW_EM_KMAX];
};

static inline PenArgs pen_args(const arflow_penalty_t* p) {
  PenArgs a;
  a.k = p->k;
  for (int j = 0; j < ARFLOW_EM_KMAX; ++j) a.w[j] = p->w[j], a.beta[j] = p->beta[j];
  return a;
}

// what every penalised entry point requires of its descriptor; census: a data-term call (takes GMM, not GMM_SQ)
static inline int pen_check(const arflow_penalty_t* p, bool census) {
  AF_REQUIRE_PTR(p);
  AF_REQUIRE(p->kind >= ARFLOW_PEN_IDENTITY && p->kind <= ARFLOW_PEN_GMM_SQ, ARFLOW_EPARAM);
  AF_REQUIRE(p->kind != (census ? ARFLOW_PEN_GMM_SQ : ARFLOW_PEN_GMM), ARFLOW_EPARAM);
  if (p->kind == ARFLOW_PEN_GMM || p->kind == ARFLOW_PEN_GMM_SQ) {
    AF_REQUIRE(p->k >= 1 && p->k <= ARFLOW_EM_KMAX, ARFLOW_EPARAM);
    int widest = 0;  // the component with the smallest beta (among equals, the heaviest)
    for (int j = 0; j < p->k; ++j) {
      AF_REQUIRE(std::isfinite(p->beta[j]) && p->beta[j] > 0.f, ARFLOW_EPARAM);
      AF_REQUIRE(std::isfinite(p->w[j]) && p->w[j] >= 0.f, ARFLOW_EPARAM);
      if (p->beta[j] < p->beta[widest] || (p->beta[j] == p->beta[widest] && p->w[j] > p->w[widest])) widest = j;
    }
    // its argument is the maximum c for every x, so e = 1 and den >= its weight: with that weight positive the density never
    // underflows to 0 (rho = inf, rho' = NaN, and NaN x 0 at a masked pixel would poison the sums)
    AF_REQUIRE(p->w[widest] > 0.f, ARFLOW_EPARAM);
  }
  return ARFLOW_OK;
}

// Runs f(std::integral_constant<int, KIND>) for a checked kind
template <class F>
static inline void pen_dispatch_kind(int kind, F&& f) {
  switch (kind) {
    case ARFLOW_PEN_IDENTITY: f(std::integral_constant<int, ARFLOW_PEN_IDENTITY>{}); break;
    case ARFLOW_PEN_CHARBONNIER: f(std::integral_constant<int, ARFLOW_PEN_CHARBONNIER>{}); break;
    case ARFLOW_PEN_ABS_ROBUST: f(std::integral_constant<int, ARFLOW_PEN_ABS_ROBUST>{}); break;
    case ARFLOW_PEN_GMM: f(std::integral_constant<int, ARFLOW_PEN_GMM>{}); break;
    default: f(std::integral_constant<int, ARFLOW_PEN_GMM_SQ>{}); break;
  }
}

constexpr float PEN_CHARB_EPS2 = 1e-6f;                                   // eps^2, eps = 0.001
constexpr float PEN_AR_EPS = 0.01f, PEN_AR_POW = 0.4f, PEN_AR_DPOW = -0.6f;  // abs_robust_loss and its exponent - 1

// the mixture in the reference's order; SQ: the argument is already a square
template <bool SQ>
__device__ __forceinline__ void pen_mixture(const PenArgs& P, float x, float& rho, float& drho) {
  const float q = SQ ? x : x * x;
  float c = (-P.beta[0] * q) / 2.f;
#pragma unroll 1
  for (int j = 1; j < P.k; ++j) c = fmaxf(c, (-P.beta[j] * q) / 2.f);
  float den = 0.f, num = 0.f;
#pragma unroll 1
  for (int j = 0; j < P.k; ++j) {
    const float t = P.w[j] * expf((-P.beta[j] * q) / 2.f - c);
    den += t;
    num += t * P.beta[j];
  }
  rho = -(c + logf(den));
  drho = SQ ? (num / den) / 2.f : (num / den) * x;
}

// rho(x) and rho'(x) of one kind
template <int KIND>
__device__ __forceinline__ void pen_rho(const PenArgs& P, float x, float& rho, float& drho) {
  if constexpr (KIND == ARFLOW_PEN_IDENTITY) {
    rho = x, drho = 1.f;
  } else if constexpr (KIND == ARFLOW_PEN_CHARBONNIER) {
    rho = sqrtf(x + PEN_CHARB_EPS2);
    drho = 0.5f / rho;
  } else if constexpr (KIND == ARFLOW_PEN_ABS_ROBUST) {
    const float lg = __log2f(fabsf(x) + PEN_AR_EPS);
    rho = exp2f(PEN_AR_POW * lg);
    drho = PEN_AR_POW * exp2f(PEN_AR_DPOW * lg) * (x < 0.f ? -1.f : 1.f);
  } else {
    pen_mixture<KIND == ARFLOW_PEN_GMM_SQ>(P, x, rho, drho);
  }
}

}  // namespace
