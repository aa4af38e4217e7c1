// The penalised census forwards of UFlowElboLoss: the fused photometric direction (single and pair
// form) and the standalone census reduction with the epilogue rho of penalty_dev.hpp in place of abs_robust_loss, and an
// optional second flow for mask_invalid (occ_type 'mean').  New kernels next to the unpenalised ones: fwd_col_kernel
// (census_col.hip) and the census forwards of photo.hip keep the code they have.
//
// The fused forwards always run the column family (census_col.hpp): tile fill and pair loop are its fill_tiles /
// pair_sums_fwd, only the epilogue differs.  The saved plane keeps its meaning dham = pm rho'(ham), so every census backward
// entry point serves every kind.
#include "census_col.hpp"
#include "penalty_dev.hpp"

namespace {
namespace census_pen {

// census_loss of one pixel under penalty KIND: adds rho(s) pm and pm to the partial sums; dh = pm rho'(s).  ABS_ROBUST is
// ham_loss_terms itself, so that it stays bit for bit what the unpenalised kernels compute.
template <int KIND>
__device__ __forceinline__ void pen_loss_terms(const PenArgs& P, float s, float pm, float (&part)[2], float& dh) {
  if constexpr (KIND == ARFLOW_PEN_ABS_ROBUST) {
    ham_loss_terms(s, pm, part, dh);
  } else {
    float rho, drho;
    pen_rho<KIND>(P, s, rho, drho);
    part[0] += rho * pm;
    part[1] += pm;
    dh = pm * drho;
  }
}

// fwd_col_kernel of census_col.hip with the penalty policy and the validity flow
template <int R, int KIND>
__global__ __launch_bounds__(census_col::NT) void fwd_col_pen_kernel(
    const float* __restrict__ gray_a, const float* __restrict__ gray_b, const float* __restrict__ flow, long fbs,
    const float* __restrict__ occ_small, float* __restrict__ mask_out, float* __restrict__ dham_out, float* __restrict__ sums,
    int nrows, int nimg, int H, int W, int pair, const float* __restrict__ valid_flow, long vbs, PenArgs P) {
  namespace cc = census_col;
  __shared__ float ta[cc::TILE];
  __shared__ float tb[cc::TILE];
  __shared__ float tm[cc::TILE];
  __shared__ float tocc[cc::OCC_R * cc::OCC_P];
  __shared__ float red[2 * (cc::NT / 64)];
  int btx, bty, b;
  if (!af_tile_of_block(cc::tiles_x(W, R), cc::tiles_y(H), nimg, btx, bty, b)) {
    if (threadIdx.x == 0) af_store_partial(sums, nrows, 0.f, 0.f, 0.f);  // padding workgroup: its row must be defined
    return;
  }
  const int y0 = bty * cc::TROWS, x0 = btx * cc::Geo<R>::UX - R;
  const long cs = (long)H * W;
  const int bp = pair ? (b ^ 1) : b;
  const float* occ = occ_small ? occ_small + (long)bp * (H / 4) * (W / 4) : nullptr;
  const int ox = max(x0 + R, 0);  // first owned column
  if (occ) cc::stage_occ(tocc, occ, H / 4, W / 4, y0, ox);
  cc::fill_tiles<R, false>(ta, tb, tm, nullptr, nullptr, gray_a + b * cs, gray_b + bp * cs, flow + b * fbs, nullptr, H, W, y0,
                           x0);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float s[cc::K];
  cc::pair_sums_fwd<R>(ta, tb, w, lane, s);
  const int x = x0 + lane;
  float part[2] = {0.f, 0.f};
  if (lane >= R && x < W) {
    const float* vf = valid_flow ? valid_flow + b * vbs : nullptr;
#pragma unroll
    for (int i = 0; i < cc::K; ++i) {
      const int y = y0 + w * cc::K + i;
      if (y < H) {
        const long po = (long)y * W + x;
        // mask_invalid of the sampling flow (staged by fill_tiles) or of the validity flow; x the upsampled range map
        float mv = vf ? flow_valid(x, y, vf[po], vf[po + cs], H, W) : tm[(R + w * cc::K + i) * cc::PITCH + lane];
        if (occ) mv *= cc::up4_lds(tocc, H / 4, W / 4, y0, ox, y, x);
        float dh;
        pen_loss_terms<KIND>(P, s[i], interior(y, x, H, W, R) ? mv : 0.f, part, dh);
        const long o = (long)b * cs + po;
        if (mask_out) mask_out[o] = mv;
        dham_out[o] = dh;
      }
    }
  }
  af_block_sum<2>(part, red);
  if (threadIdx.x == 0) store_dir_partial(sums, nrows, part, pair, b);
}

// The standalone route's second launch: rho over the distances `ham` under the border-zeroed mask; one lane per pixel, a
// workgroup = 256 columns of one row (the one-thread-per-pixel grid af_sums_rows counts).
template <int KIND>
__global__ __launch_bounds__(256) void pen_apply_kernel(const float* __restrict__ ham, const float* __restrict__ mask,
                                                       float* __restrict__ dham, float* __restrict__ sums, int nrows, int H,
                                                       int W, int R, PenArgs P) {
  __shared__ float red[2 * 4];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  float part[2] = {0.f, 0.f};
  if (x < W) {
    const long o = ((long)b * H + y) * W + x;
    float dh;
    pen_loss_terms<KIND>(P, ham[o], interior(y, x, H, W, R) ? mask[o] : 0.f, part, dh);
    dham[o] = dh;
  }
  af_block_sum<2>(part, red);
  if (threadIdx.x == 0) af_store_partial(sums, nrows, part[0], part[1], 0.f);
}

}  // namespace census_pen
}  // namespace

static int census_warp_pen_fwd_impl(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                    const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H, int W,
                                    int radius, const float* valid_flow, long valid_bstride, const arflow_penalty_t* pen,
                                    arflow_stream_t stream, int pair) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(gray_a);
  AF_REQUIRE_PTR(gray_b);
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(dham);
  AF_REQUIRE_PTR(sums);
  AF_REQUIRE_PTR(pen);
  AF_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 8 * 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(arflow_census_warp_supported(H, W), ARFLOW_ESHAPE);
  AF_REQUIRE(flow_bstride >= 2L * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(!valid_flow || valid_bstride >= 2L * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(!pair || B % 2 == 0, ARFLOW_ESHAPE);
  AF_REQUIRE(radius >= 1 && radius <= 3, ARFLOW_EPARAM);
  if (const int rc = pen_check(pen, true)) return rc;
  namespace cp = census_pen;
  const PenArgs P = pen_args(pen);
  const int nrows = af_sums_rows(B, H, W);
  const dim3 g(af_grid_for_tiles((long)census_col::tiles_x(W, radius) * census_col::tiles_y(H) * B)), t(census_col::NT);
  af_dispatch_radius(radius, [&](auto R) {
    pen_dispatch_kind(pen->kind, [&](auto KIND) {
      if constexpr (decltype(KIND)::value != ARFLOW_PEN_GMM_SQ)
        hipLaunchKernelGGL((cp::fwd_col_pen_kernel<decltype(R)::value, decltype(KIND)::value>), g, t, 0, (hipStream_t)stream,
                           gray_a, gray_b, flow, flow_bstride, occ_small, mask_out, dham, sums, nrows, B, H, W, pair, valid_flow,
                           valid_bstride, P);
    });
  });
  return af_launch_status();
}

extern "C" int arflow_census_warp_pen_fwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                          const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H,
                                          int W, int radius, const float* valid_flow, long valid_bstride,
                                          const arflow_penalty_t* pen, arflow_stream_t stream) {
  return census_warp_pen_fwd_impl(gray_a, gray_b, flow, flow_bstride, occ_small, mask_out, dham, sums, B, H, W, radius,
                                  valid_flow, valid_bstride, pen, stream, 0);
}

extern "C" int arflow_census_warp_pair_pen_fwd(const float* gray, const float* flow, long flow_bstride, const float* occ_small,
                                               float* mask_out, float* dham, float* sums, int B2, int H, int W, int radius,
                                               const float* valid_flow, long valid_bstride, const arflow_penalty_t* pen,
                                               arflow_stream_t stream) {
  return census_warp_pen_fwd_impl(gray, gray, flow, flow_bstride, occ_small, mask_out, dham, sums, B2, H, W, radius, valid_flow,
                                  valid_bstride, pen, stream, 1);
}

extern "C" int arflow_census_pen_fwd(const float* im_a, const float* im_b, const float* mask, float* ham, float* dham,
                                     float* sums, int B, int H, int W, int radius, const arflow_penalty_t* pen,
                                     arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(im_a);
  AF_REQUIRE_PTR(im_b);
  AF_REQUIRE_PTR(mask);
  AF_REQUIRE_PTR(ham);
  AF_REQUIRE_PTR(dham);
  AF_REQUIRE_PTR(sums);
  AF_REQUIRE_PTR(pen);
  AF_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(radius >= 1 && radius <= 3, ARFLOW_EPARAM);
  if (const int rc = pen_check(pen, true)) return rc;
  if (const int rc = arflow_census_fwd(im_a, im_b, nullptr, ham, nullptr, nullptr, B, H, W, radius, stream)) return rc;
  namespace cp = census_pen;
  const PenArgs P = pen_args(pen);
  const int nrows = af_sums_rows(B, H, W);
  pen_dispatch_kind(pen->kind, [&](auto KIND) {
    if constexpr (decltype(KIND)::value != ARFLOW_PEN_GMM_SQ)
      hipLaunchKernelGGL(cp::pen_apply_kernel<decltype(KIND)::value>, dim3(af_cdiv(W, 256), H, B), dim3(256), 0,
                         (hipStream_t)stream, ham, mask, dham, sums, nrows, H, W, radius, P);
  });
  return af_launch_status();
}
