// Edge-aware smoothness with a selectable penalty (UFlowElboLoss's sampled smoothness, losses/uflow_elbo_loss.py:507-533):
// smooth.hip's forward and backward with rho of penalty_dev.hpp applied to x = v^2 of the signed difference v,
// d rho / d v = 2 v rho'(x).  Launch shapes, edge weights, differences and the order of every addition are smooth.hip's
// (smooth_dev.hpp); CHARBONNIER is pen(v, 1) / dpen(v, 1) themselves, so it equals arflow_smooth_fwd / _bwd(penalty = 1) bit
// for bit.  DESIGN.md section 45.
#include "penalty_dev.hpp"
#include "smooth_dev.hpp"

namespace {
namespace smooth_pen {

template <int KIND>
__device__ __forceinline__ float pval(const PenArgs& P, float v) {
  if constexpr (KIND == ARFLOW_PEN_CHARBONNIER) {
    return pen(v, 1);
  } else {
    float rho, drho;
    pen_rho<KIND>(P, v * v, rho, drho);
    return rho;
  }
}
template <int KIND>
__device__ __forceinline__ float pder(const PenArgs& P, float v) {
  if constexpr (KIND == ARFLOW_PEN_CHARBONNIER) {
    return dpen(v, 1);
  } else {
    float rho, drho;
    pen_rho<KIND>(P, v * v, rho, drho);
    return (2.f * v) * drho;
  }
}

// smooth_fwd_kernel of smooth.hip under penalty KIND
template <int CI, int KIND>
__global__ __launch_bounds__(256) void fwd_kernel(SmoothArgs a, float* __restrict__ sums, int nrows, int rows, PenArgs P) {
  __shared__ float red[2 * 4];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
  const int o = a.order;
  float part[2] = {0.f, 0.f};
  if (x < a.W) {
    const float* ib = a.img + (long)b * a.Ci * a.H * a.W;
    const float* fb = a.flow + (long)b * a.fbs;
    const long cs = (long)a.H * a.W;
    for (int r = 0; r < rows; ++r) {
      const int y = blockIdx.y * rows + r;
      if (y >= a.H) break;
      if (x < a.W - o) {
        const float w = edge_wx<CI>(a, ib, y, x);
        part[0] += w * (pval<KIND>(P, diff_x(a, fb, y, x)) + pval<KIND>(P, diff_x(a, fb + cs, y, x)));
      }
      if (y < a.H - o) {
        const float w = edge_wy<CI>(a, ib, y, x);
        part[1] += w * (pval<KIND>(P, diff_y(a, fb, y, x)) + pval<KIND>(P, diff_y(a, fb + cs, y, x)));
      }
    }
  }
  af_block_sum<2>(part, red);
  if (threadIdx.x == 0) af_store_partial(sums, nrows, part[0], part[1], 0.f);
}

// smooth_bwd_pixel of smooth_dev.hpp under penalty KIND
template <int CI, int KIND>
__global__ __launch_bounds__(256) void bwd_kernel(SmoothArgs a, const float* __restrict__ coef, float* __restrict__ gflow,
                                                 PenArgs P) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= a.W) return;
  const int o = a.order;
  const float* ib = a.img + (long)b * a.Ci * a.H * a.W;
  const float* fb = a.flow + (long)b * a.fbs;
  const long cs = (long)a.H * a.W;
  const float cx = coef[0] * a.fscale, cy = coef[1] * a.fscale;
  float g[2] = {0.f, 0.f};
  const float st1[2] = {-1.f, 1.f};
  const float st2[3] = {1.f, -2.f, 1.f};
  for (int k = 0; k <= o; ++k) {
    const float s = o == 1 ? st1[k] : st2[k];
    const int xa = x - k;
    if (xa >= 0 && xa < a.W - o) {
      const float w = edge_wx<CI>(a, ib, y, xa) * s * cx;
      g[0] = fmaf(w, pder<KIND>(P, diff_x(a, fb, y, xa)), g[0]);
      g[1] = fmaf(w, pder<KIND>(P, diff_x(a, fb + cs, y, xa)), g[1]);
    }
    const int ya = y - k;
    if (ya >= 0 && ya < a.H - o) {
      const float w = edge_wy<CI>(a, ib, ya, x) * s * cy;
      g[0] = fmaf(w, pder<KIND>(P, diff_y(a, fb, ya, x)), g[0]);
      g[1] = fmaf(w, pder<KIND>(P, diff_y(a, fb + cs, ya, x)), g[1]);
    }
  }
  float* go = gflow + (long)b * 2 * cs + (long)y * a.W + x;
  go[0] = g[0];
  go[cs] = g[1];
}

int check(const float* flow, const float* img, int B, int Ci, int H, int W, long fbs, int order, int wmode) {
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(img);
  AF_REQUIRE(B > 0 && Ci > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(fbs >= 2L * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(order == 1 || order == 2, ARFLOW_EPARAM);
  AF_REQUIRE(wmode == 0 || wmode == 1, ARFLOW_EPARAM);
  return ARFLOW_OK;
}

}  // namespace smooth_pen
}  // namespace

extern "C" int arflow_smooth_pen_fwd(const float* flow, const float* img, float* sums, int B, int Ci, int H, int W,
                                     long flow_bstride, float flow_scale, float alpha, int order, int wmode,
                                     const arflow_penalty_t* pen, arflow_stream_t stream) {
  af_clear_stale_error();
  namespace sp = smooth_pen;
  if (const int rc = sp::check(flow, img, B, Ci, H, W, flow_bstride, order, wmode)) return rc;
  AF_REQUIRE_PTR(sums);
  if (const int rc = pen_check(pen, false)) return rc;
  const PenArgs P = pen_args(pen);
  const int nrows = af_sums_rows(B, H, W);
  const SmoothArgs a{flow, img, Ci, H, W, flow_bstride, flow_scale, alpha, order, wmode, 1};
  long rows = (long)af_cdiv(W, 256) * H * B / 2048;
  rows = rows < 1 ? 1 : (rows > 8 ? 8 : rows);
  const dim3 grid(af_cdiv(W, 256), af_cdiv(H, rows), B);
  pen_dispatch_kind(pen->kind, [&](auto KIND) {
    constexpr int KD = decltype(KIND)::value;
    if constexpr (KD != ARFLOW_PEN_GMM) {
      if (Ci == 3)
        hipLaunchKernelGGL((sp::fwd_kernel<3, KD>), grid, dim3(256), 0, (hipStream_t)stream, a, sums, nrows, (int)rows, P);
      else
        hipLaunchKernelGGL((sp::fwd_kernel<0, KD>), grid, dim3(256), 0, (hipStream_t)stream, a, sums, nrows, (int)rows, P);
    }
  });
  return af_launch_status();
}

extern "C" int arflow_smooth_pen_bwd(const float* flow, const float* img, const float* coef, float* gflow, int B, int Ci, int H,
                                     int W, long flow_bstride, float flow_scale, float alpha, int order, int wmode,
                                     const arflow_penalty_t* pen, arflow_stream_t stream) {
  af_clear_stale_error();
  namespace sp = smooth_pen;
  if (const int rc = sp::check(flow, img, B, Ci, H, W, flow_bstride, order, wmode)) return rc;
  AF_REQUIRE_PTR(coef);
  AF_REQUIRE_PTR(gflow);
  if (const int rc = pen_check(pen, false)) return rc;
  const PenArgs P = pen_args(pen);
  const SmoothArgs a{flow, img, Ci, H, W, flow_bstride, flow_scale, alpha, order, wmode, 1};
  const dim3 grid(af_cdiv(W, 256), H, B);
  pen_dispatch_kind(pen->kind, [&](auto KIND) {
    constexpr int KD = decltype(KIND)::value;
    if constexpr (KD != ARFLOW_PEN_GMM) {
      if (Ci == 3)
        hipLaunchKernelGGL((sp::bwd_kernel<3, KD>), grid, dim3(256), 0, (hipStream_t)stream, a, coef, gflow, P);
      else
        hipLaunchKernelGGL((sp::bwd_kernel<0, KD>), grid, dim3(256), 0, (hipStream_t)stream, a, coef, gflow, P);
    }
  });
  return af_launch_status();
}
