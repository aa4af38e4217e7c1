// Fused optimiser step over the flat gradient buffer of ddp.FlatGradAllReduce: ONE launch updates every
// parameter of the model, whatever its group, from a chunk table in device memory; one more launch in front of it when the
// global gradient norm is needed (clipping, or the non-finite guard).
//   trainer/base_trainer.py:78-129 (the three optimisers and their two decay groups), trainer/uflow_elbo_trainer.py:94-99
//   (clip_grad_norm_ in front of the step), utils/torch_utils.py:82-161 (the reference's own AdamW).
// The flat buffers grad, s1 (exp_avg, or momentum_buffer) and s2 (exp_avg_sq) share ONE layout; the parameters stay where torch
// allocated them, a table row names the address.  Row r (ARFLOW_OPTIM_ROW 64-bit words): parameter address, flat offset, count
// (1 .. ARFLOW_OPTIM_CHUNK) and the weight decay of the row's group as the bits of a double.  One workgroup per row.
//
// NORM.  arflow_optim_gradnorm: workgroup b sums g^2 over elements [b per, (b + 1) per) in float64 (the square of an fp32 number
// is exact there; af_block_sum_f64) and STORES one partial.  No atomics, no zero-fill: two calls give the same bits, in either
// mode.  The step kernel adds the partials in index order to 0.0 and forms, in float64,
//     total_norm = sqrt(sum)      coef = clip > 0 ? min(1, clip / (total_norm + 1e-6)) : 1      (torch.nn.utils.clip_grad_norm_)
// coef is rounded to fp32 once and multiplies the gradient AS IT IS READ; the stored gradient is not rewritten (the reference
// rewrites .grad; nobody reads it between the clip and the next zero_grad).  Without partials coef = 1.
// GUARD.  With the guard on and total_norm not finite no parameter or state element is written and lane 0 of workgroup 0 adds
// one to *skipped (a plain load and store: it is the only writer).
//
// SCALARS arrive as doubles and are rounded to fp32 ONCE, here:  b1 = fl(beta1), c1 = fl(1 - beta1), b2 = fl(beta2),
// c2 = fl(1 - beta2), e = fl(eps), wd = fl(weight decay), lr = fl(lr), s2c = fl(sqrt(1 - beta2^t)), and the step sizes below
// (1 - beta, lr / bc1 and lr sqrt(bc2) / bc1 are formed in float64 first).  bc1 = 1 - beta1^t.
// THE FP32 OPERATION ORDER of one element (every operation rounds once: -ffp-contract=off, IEEE division and square root):
//     g = coef * grad
//   adam   (torch.optim.Adam, L2 decay)            adamw  (the reference's class)              sgd  (torch.optim.SGD, momentum mu)
//     g = g + wd * p         [wd != 0]               --                                          g = g + wd * p       [wd != 0]
//     m = b1 * m + c1 * g                            the same                                    buf = first ? g : mu * buf + g
//     v = b2 * v + c2 * (g * g)                      the same
//     d = sqrt(v) / s2c + e                          d = sqrt(v) + e
//     p = p - fl(lr / bc1) * (m / d)                 p = p - fl(lr sqrt(bc2) / bc1) * (m / d)    p = p - lr * buf
//                                                    p = p - wd * p      [wd != 0; NOT scaled by lr]
// float4 accesses where the parameter address, the three flat addresses of the row and the count allow it; the scalar path is
// the same template and complete: behind a 2-element head bias every later flat offset is off the 16-byte grid.
#include "common.hpp"

#include <cmath>

namespace {

constexpr int OP_NT = 256;
constexpr int OP_CHUNK = ARFLOW_OPTIM_CHUNK;
constexpr int OP_PER_LANE = OP_CHUNK / OP_NT;  // 8 elements of each stream per lane
constexpr long OP_NORM_UNIT = 4096;            // a norm workgroup's share is a multiple of this
constexpr int OP_MAX_PARTS = 256;
constexpr int OP_NORM_ILP = 8;  // float4 loads a lane of the norm kernel keeps in flight
static_assert(OP_CHUNK % (4 * OP_NT) == 0, "a chunk is whole float4 trips of the workgroup");

inline long op_norm_share(long n) {
  const long units = (n + OP_NORM_UNIT - 1) / OP_NORM_UNIT;
  return OP_NORM_UNIT * ((units + OP_MAX_PARTS - 1) / OP_MAX_PARTS);
}
inline int op_partials(long n) {
  const long per = op_norm_share(n);
  return (int)((n + per - 1) / per);
}

template <bool VEC>
__global__ __launch_bounds__(OP_NT) void optim_gradnorm_kernel(const float* __restrict__ g, double* __restrict__ part, long n, long per) {
  __shared__ double scratch[OP_NT / AF_WAVE];
  const long lo = (long)blockIdx.x * per, hi = min(lo + per, n);
  double acc[1] = {0.0};
  long i = lo + 4 * (long)threadIdx.x;
  if (VEC) {  // whole trips of OP_NORM_ILP float4 per lane, every load in flight before the first square (a fixed order too)
    for (; i + 4 * OP_NT * (OP_NORM_ILP - 1) + 3 < hi; i += 4 * OP_NT * OP_NORM_ILP) {
      float4 t[OP_NORM_ILP];
#pragma unroll
      for (int k = 0; k < OP_NORM_ILP; ++k) t[k] = *reinterpret_cast<const float4*>(g + i + 4 * OP_NT * k);
#pragma unroll
      for (int k = 0; k < OP_NORM_ILP; ++k)
        acc[0] += ((double)t[k].x * (double)t[k].x + (double)t[k].y * (double)t[k].y) +
                  ((double)t[k].z * (double)t[k].z + (double)t[k].w * (double)t[k].w);
    }
  }
  for (; i < hi; i += 4 * OP_NT) {
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC && i + 3 < hi) {
      const float4 t = *reinterpret_cast<const float4*>(g + i);
      x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < hi) x[j] = g[i + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[0] += (double)x[j] * (double)x[j];
  }
  af_block_sum_f64<1, OP_NT>(acc, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

struct OpArgs {
  const long long* table;
  const float* grad;
  float* s1;
  float* s2;
  const double* part;
  int* skipped;
  long n;
  int nrows, nparts, guard, first;
  double clip, lr, bc1, sqbc2, eps, beta1, beta2;
};

// the scalars of a launch in fp32
struct OpScal {
  float coef, b1, c1, b2, c2, eps, lr, s2c, step;
};

template <int RULE>
__device__ __forceinline__ void op_element(const OpScal& k, float wd, bool first, float graw, float& p, float& m, float& v) {
  float g = k.coef * graw;
  if (RULE != ARFLOW_OPTIM_ADAMW && wd != 0.f) g = g + wd * p;
  if (RULE == ARFLOW_OPTIM_SGD) {
    m = first ? g : k.b1 * m + g;
    p = p - k.lr * m;
    return;
  }
  m = k.b1 * m + k.c1 * g;
  v = k.b2 * v + k.c2 * (g * g);
  const float d = RULE == ARFLOW_OPTIM_ADAM ? sqrtf(v) / k.s2c + k.eps : sqrtf(v) + k.eps;
  p = p - k.step * (m / d);
  if (RULE == ARFLOW_OPTIM_ADAMW && wd != 0.f) p = p - wd * p;
}

// one row: OP_PER_LANE elements per lane, every load of the row in flight before the first store
template <int RULE, bool VEC>
__device__ __forceinline__ void op_row(const OpScal& k, float wd, bool first, float* __restrict__ P, const float* __restrict__ G,
                                       float* __restrict__ S1, float* __restrict__ S2, int cnt) {
  constexpr bool TWO = RULE != ARFLOW_OPTIM_SGD;
  if (VEC) {
    constexpr int TRIPS = OP_PER_LANE / 4;
    float4 p[TRIPS], g[TRIPS], m[TRIPS], v[TRIPS];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int i = 4 * (t * OP_NT + (int)threadIdx.x);
      if (i < cnt) {
        p[t] = *reinterpret_cast<const float4*>(P + i);
        g[t] = *reinterpret_cast<const float4*>(G + i);
        m[t] = *reinterpret_cast<const float4*>(S1 + i);
        if (TWO) v[t] = *reinterpret_cast<const float4*>(S2 + i);
      }
    }
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int i = 4 * (t * OP_NT + (int)threadIdx.x);
      if (i < cnt) {
        op_element<RULE>(k, wd, first, g[t].x, p[t].x, m[t].x, v[t].x);
        op_element<RULE>(k, wd, first, g[t].y, p[t].y, m[t].y, v[t].y);
        op_element<RULE>(k, wd, first, g[t].z, p[t].z, m[t].z, v[t].z);
        op_element<RULE>(k, wd, first, g[t].w, p[t].w, m[t].w, v[t].w);
        *reinterpret_cast<float4*>(P + i) = p[t];
        *reinterpret_cast<float4*>(S1 + i) = m[t];
        if (TWO) *reinterpret_cast<float4*>(S2 + i) = v[t];
      }
    }
  } else {
    float p[OP_PER_LANE], g[OP_PER_LANE], m[OP_PER_LANE], v[OP_PER_LANE];
#pragma unroll
    for (int t = 0; t < OP_PER_LANE; ++t) {
      const int i = t * OP_NT + (int)threadIdx.x;
      if (i < cnt) {
        p[t] = P[i], g[t] = G[i], m[t] = S1[i];
        if (TWO) v[t] = S2[i];
      }
    }
#pragma unroll
    for (int t = 0; t < OP_PER_LANE; ++t) {
      const int i = t * OP_NT + (int)threadIdx.x;
      if (i < cnt) {
        op_element<RULE>(k, wd, first, g[t], p[t], m[t], v[t]);
        P[i] = p[t], S1[i] = m[t];
        if (TWO) S2[i] = v[t];
      }
    }
  }
}

template <int RULE>
__global__ __launch_bounds__(OP_NT) void optim_step_kernel(const OpArgs a) {
  __shared__ double sum_s;
  OpScal k;
  k.coef = 1.0f;
  if (a.nparts > 0) {  // uniform over the grid
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < a.nparts; ++i) s += a.part[i];
      sum_s = s;
    }
    __syncthreads();
    const double total = sqrt(sum_s);
    if (a.guard && !isfinite(total)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) *a.skipped = *a.skipped + 1;
      return;
    }
    if (a.clip > 0.0) k.coef = (float)fmin(1.0, a.clip / (total + 1e-6));
  }
  k.b1 = (float)a.beta1, k.c1 = (float)(1.0 - a.beta1), k.b2 = (float)a.beta2, k.c2 = (float)(1.0 - a.beta2);
  k.eps = (float)a.eps, k.lr = (float)a.lr, k.s2c = (float)a.sqbc2;
  k.step = RULE == ARFLOW_OPTIM_ADAM ? (float)(a.lr / a.bc1) : (float)(a.lr * a.sqbc2 / a.bc1);

  const long long* row = a.table + (long)blockIdx.x * ARFLOW_OPTIM_ROW;
  float* P = reinterpret_cast<float*>((uintptr_t)row[ARFLOW_OPTIM_ADDR]);
  const long off = (long)row[ARFLOW_OPTIM_OFFSET];
  const long cnt = (long)row[ARFLOW_OPTIM_COUNT];
  const float wd = (float)__longlong_as_double(row[ARFLOW_OPTIM_DECAY]);
  // a row that leaves the flat buffers is not run; the ADDRESS cannot be checked here: the host compares it before every step
  if (P == nullptr || off < 0 || cnt < 1 || cnt > OP_CHUNK || off > a.n - cnt) return;
  const float* G = a.grad + off;
  float* S1 = a.s1 + off;
  float* S2 = RULE != ARFLOW_OPTIM_SGD ? a.s2 + off : nullptr;
  const bool vec = cnt % 4 == 0 && (((uintptr_t)P | (uintptr_t)G | (uintptr_t)S1 | (uintptr_t)S2) & 15) == 0;
  if (vec)
    op_row<RULE, true>(k, wd, a.first != 0, P, G, S1, S2, (int)cnt);
  else
    op_row<RULE, false>(k, wd, a.first != 0, P, G, S1, S2, (int)cnt);
}

inline bool op_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int arflow_optim_partials(long n) {
  AF_REQUIRE(n >= 1, ARFLOW_ESHAPE);
  return op_partials(n);
}

extern "C" int arflow_optim_gradnorm(const float* grad, double* partials, long n, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(grad);
  AF_REQUIRE_PTR(partials);
  AF_REQUIRE(n >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(op_aligned4(grad) && ((uintptr_t)partials & 7) == 0, ARFLOW_EPARAM);
  const long per = op_norm_share(n);
  const dim3 grid((unsigned)op_partials(n));
  if (af_aligned16(grad))
    hipLaunchKernelGGL(optim_gradnorm_kernel<true>, grid, dim3(OP_NT), 0, (hipStream_t)stream, grad, partials, n, per);
  else
    hipLaunchKernelGGL(optim_gradnorm_kernel<false>, grid, dim3(OP_NT), 0, (hipStream_t)stream, grad, partials, n, per);
  return af_launch_status();
}

extern "C" int arflow_optim_step(const long long* table, int nrows, const float* grad, float* s1, float* s2, long n,
                                 const double* partials, int nparts, int* skipped, int rule, int first, double lr, double bc1,
                                 double sqbc2, double eps, double beta1, double beta2, double clip, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(table);
  AF_REQUIRE_PTR(grad);
  AF_REQUIRE_PTR(s1);
  AF_REQUIRE(rule == ARFLOW_OPTIM_ADAM || rule == ARFLOW_OPTIM_ADAMW || rule == ARFLOW_OPTIM_SGD, ARFLOW_EPARAM);
  if (rule != ARFLOW_OPTIM_SGD) AF_REQUIRE_PTR(s2);
  AF_REQUIRE(nrows >= 1 && n >= 1, ARFLOW_ESHAPE);
  // the norm is either absent or exactly what arflow_optim_gradnorm stored for this n
  AF_REQUIRE(nparts == 0 || nparts == op_partials(n), ARFLOW_ESHAPE);
  if (nparts > 0) AF_REQUIRE_PTR(partials);
  AF_REQUIRE(first == 0 || first == 1, ARFLOW_EPARAM);
  AF_REQUIRE(std::isfinite(lr) && std::isfinite(clip), ARFLOW_EPARAM);
  AF_REQUIRE((clip <= 0.0 && skipped == nullptr) || nparts > 0, ARFLOW_EPARAM);  // clipping and the guard need the norm
  AF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, ARFLOW_EPARAM);
  if (rule != ARFLOW_OPTIM_SGD)
    AF_REQUIRE(beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && std::isfinite(eps) && bc1 > 0.0 && bc1 <= 1.0 && sqbc2 > 0.0 && sqbc2 <= 1.0,
               ARFLOW_EPARAM);
  AF_REQUIRE(((uintptr_t)table & 7) == 0 && op_aligned4(grad) && op_aligned4(s1) && op_aligned4(s2) && op_aligned4(skipped) &&
                 ((uintptr_t)partials & 7) == 0,
             ARFLOW_EPARAM);
  OpArgs a = {};
  a.table = table, a.grad = grad, a.s1 = s1, a.s2 = s2, a.part = partials, a.skipped = skipped;
  a.n = n, a.nrows = nrows, a.nparts = nparts, a.guard = skipped != nullptr, a.first = first;
  a.clip = clip, a.lr = lr, a.bc1 = bc1, a.sqbc2 = sqbc2, a.eps = eps, a.beta1 = beta1, a.beta2 = beta2;
  const dim3 grid((unsigned)nrows);
  switch (rule) {
    case ARFLOW_OPTIM_ADAM: hipLaunchKernelGGL(optim_step_kernel<ARFLOW_OPTIM_ADAM>, grid, dim3(OP_NT), 0, (hipStream_t)stream, a); break;
    case ARFLOW_OPTIM_ADAMW: hipLaunchKernelGGL(optim_step_kernel<ARFLOW_OPTIM_ADAMW>, grid, dim3(OP_NT), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(optim_step_kernel<ARFLOW_OPTIM_SGD>, grid, dim3(OP_NT), 0, (hipStream_t)stream, a); break;
  }
  return af_launch_status();
}
