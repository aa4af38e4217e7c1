// Ground-truth flow metrics in one launch: the per-sample sums behind evaluate_flow of
// utils/flow_utils.py:121-183 (EPE, E_noc, E_occ, F1_all, moving / static EPE), which trainer/uflow_trainer.py:94-170 calls
// after every epoch.  The reference copies the full-resolution prediction to the host and runs cv2.resize + numpy per
// sample; here the prediction is scaled, resized to the ground-truth size, compared and reduced where it lies, and the
// host reads B x 8 doubles whenever it wants them.
//
// Per ground-truth pixel, fp32, in the reference's order (flow_utils.py:137-146):
//   taps   u = (pred_u / w) * W,  v = (pred_v / h) * H                       scaled BEFORE the resize
//   resize bilinear, half-pixel rule (cv2.INTER_LINEAR = ATen upsample_bilinear2d(align_corners=False) with a size given):
//          up_source / up_blend of upsample_dev.hpp, the device code of upsample.hip and of the level's x2 upsample
//   epe  = sqrt(du^2 + dv^2) against gt[:, 0:2];  valid = gt[:, 2], noc = gt[:, 3] (both 1 when C = 2)
//   bad  = (e > 3) && (e / max(|gt|, 1e-10) > 0.05),  e = epe * valid          (flow_utils.py:123-128)
// The resize grid is separable: a lane's four columns fix x0, x1 and their weights once, a tile row fixes y0, y1 once.
// The prediction taps are read directly (the prediction is 2 h w floats against C H W; the taps of neighbouring pixels
// share cache lines).
//
// One 32 x 64 tile per workgroup, one row of 8 doubles per tile ([B][rows][8], rows = tiles per sample): every row of the
// buffer is stored by exactly one workgroup -- no atomics, no zero-fill, bitwise reproducible.  Partials are fp32 per
// thread over its 8 pixels and double from the wave reduction on (as featnorm.hip).
#include "common.hpp"
#include "taps.hpp"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int TW = 64, TH = 32;    // tile of ground-truth pixels
constexpr int CPT = 4;             // consecutive columns per thread (one float4: af_ld_cols4 / af_st_cols4, zeros beyond W)
constexpr int RSTEP = NT / (TW / CPT);  // tile rows per pass of the workgroup: 16
constexpr int NQ = 7;              // quantities summed (column 7 of a row is 0)
constexpr int MAX_DIM = 16384;

// grid (tile columns, tile rows, B)
template <bool VEC>
__global__ __launch_bounds__(NT) void flow_eval_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const float* __restrict__ move, double* __restrict__ rows,
                                                       float* __restrict__ epe_map, int h, int w, int C, int H, int W) {
  __shared__ double scratch[NQ * (NT / 64)];
  const int b = blockIdx.z;
  const int X0 = blockIdx.x * TW + (threadIdx.x % (TW / CPT)) * CPT;
  const int Yb = blockIdx.y * TH + threadIdx.x / (TW / CPT);
  const long HW = (long)H * W, hw = (long)h * w;
  const float* pu = pred + 2 * hw * b;
  const float* pv = pu + hw;
  const float* g = gt + C * HW * b;
  const float* mv = move ? move + HW * b : nullptr;
  float* em = epe_map ? epe_map + HW * b : nullptr;
  const float fw = (float)w, fW = (float)W, fh = (float)h, fH = (float)H;

  int xa[CPT], xb[CPT];
  float wx0[CPT], wx1[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) up_source(min(X0 + j, W - 1), w, W, fw / fW, false, xa[j], xb[j], wx0[j], wx1[j]);

  float s[NQ] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < TH / RSTEP; ++k) {
    const int Y = Yb + k * RSTEP;
    if (Y >= H) break;
    int ya, yb;
    float wy0, wy1;
    up_source(Y, h, H, fh / fH, false, ya, yb, wy0, wy1);
    const float* gr = g + (long)Y * W;
    float gu[CPT], gv[CPT], va[CPT], no[CPT], mo[CPT], epe[CPT];
    af_ld_cols4<VEC>(gr, X0, W, 0.f, gu);
    af_ld_cols4<VEC>(gr + HW, X0, W, 0.f, gv);
    if (C == 4) {
      af_ld_cols4<VEC>(gr + 2 * HW, X0, W, 0.f, va);
      af_ld_cols4<VEC>(gr + 3 * HW, X0, W, 0.f, no);
    } else {
#pragma unroll
      for (int j = 0; j < CPT; ++j) va[j] = no[j] = X0 + j < W ? 1.f : 0.f;
    }
    if (mv) {
      af_ld_cols4<VEC>(mv + (long)Y * W, X0, W, 0.f, mo);
    } else {
#pragma unroll
      for (int j = 0; j < CPT; ++j) mo[j] = 0.f;
    }
    const float* ua = pu + ya * w;
    const float* ub = pu + yb * w;
    const float* vaq = pv + ya * w;
    const float* vbq = pv + yb * w;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      // x / n for an integer n: af_div_den is the IEEE quotient in 3 instructions (common.hpp)
      const float u = up_blend(wx0[j], wx1[j], wy0, wy1, af_div_den(ua[xa[j]], fw) * fW, af_div_den(ua[xb[j]], fw) * fW,
                               af_div_den(ub[xa[j]], fw) * fW, af_div_den(ub[xb[j]], fw) * fW);
      const float v = up_blend(wx0[j], wx1[j], wy0, wy1, af_div_den(vaq[xa[j]], fh) * fH, af_div_den(vaq[xb[j]], fh) * fH,
                               af_div_den(vbq[xa[j]], fh) * fH, af_div_den(vbq[xb[j]], fh) * fH);
      const float du = u - gu[j], dv = v - gv[j];
      const bool in = X0 + j < W;  // a column beyond W took the taps of column W - 1: drop it
      epe[j] = in ? sqrtf(du * du + dv * dv) : 0.f;
      const float e = epe[j] * va[j];
      const float mag = sqrtf(gu[j] * gu[j] + gv[j] * gv[j]);
      const bool bad = e > 3.f && e / fmaxf(mag, 1e-10f) > 0.05f;
      s[0] += e;
      s[1] += va[j];
      s[2] += epe[j] * no[j];
      s[3] += no[j];
      s[4] += bad ? 1.f : 0.f;
      s[5] += e * mo[j];
      s[6] += va[j] * mo[j];
    }
    if (em) af_st_cols4<VEC>(em + (long)Y * W, X0, W, epe);
  }
  double d[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) d[q] = (double)s[q];
  af_block_sum_f64<NQ, NT>(d, scratch);
  if (threadIdx.x == 0) {
    const long tiles = (long)gridDim.x * gridDim.y;
    double* r = rows + 8 * (tiles * b + (long)blockIdx.y * gridDim.x + blockIdx.x);
#pragma unroll
    for (int q = 0; q < NQ; ++q) r[q] = d[q];
    r[7] = 0.0;
  }
}

}  // namespace

extern "C" int arflow_flow_eval_rows(int H, int W) {
  AF_REQUIRE(H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  return af_cdiv(W, TW) * af_cdiv(H, TH);
}

extern "C" int arflow_flow_eval(const float* pred, const float* gt, const float* move, double* rows, float* epe_map, int B,
                                int h, int w, int C, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(pred);
  AF_REQUIRE_PTR(gt);
  AF_REQUIRE_PTR(rows);
  AF_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(B <= 65535 && h <= MAX_DIM && w <= MAX_DIM && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  AF_REQUIRE(C == 2 || C == 4, ARFLOW_EPARAM);
  AF_REQUIRE(move == nullptr || C == 4, ARFLOW_EPARAM);
  const dim3 grid(af_cdiv(W, TW), af_cdiv(H, TH), B);
  // float4 rows of the ground-truth planes (and move / epe_map): every plane starts 16-byte aligned when W % 4 == 0
  const bool vec = W % 4 == 0 && af_aligned16(gt) && af_aligned16(move) && af_aligned16(epe_map);
  if (vec)
    hipLaunchKernelGGL(flow_eval_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, pred, gt, move, rows, epe_map, h, w, C,
                       H, W);
  else
    hipLaunchKernelGGL(flow_eval_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, pred, gt, move, rows, epe_map, h, w, C,
                       H, W);
  return af_launch_status();
}
