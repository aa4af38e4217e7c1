// Uncertainty metrics: the device side of sp_plot / evaluate_uncertainty / CalibrationCurve of
// utils/flow_utils.py:186-320, which trainer/uflow_elbo_trainer.py runs after every epoch on the entropy map that
// inverse_diagonal (triag.hip) ends in.  The reference builds a [25,H,W] float64 sigmoid stack on the host up to 11 times
// per curve and gathers 101 boolean masks per sample; here every refinement step of both curves of a whole batch is one
// streaming launch, and the histogram is one more.
//
//   arflow_uncert_prep    entropy [B,2,h,w] -> the shifted, resized, channel-summed entropy map [B,1,H,W] (fp32, in the
//                         reference's operation order, flow_utils.py:296-307), plus per tile the min / max of that map and of
//                         the end-point-error map (the bracket of sp_plot, :193-194) and sum valid.
//   arflow_sparsify_sums  for every sample, field and threshold the three sums of sp_mask / splot (:187-190, :222):
//                         sum (1-m) g, sum m g, sum err m g with m = expit(alpha (thr - field)).
//   arflow_calib_hist     count, sum e, sum e^2 of the per-channel absolute errors in the np.digitize bins of exp(entropy)
//                         (:237-254).
//
// As flow_eval.hip: every row of a row buffer is stored by exactly one workgroup -- no atomics (global or LDS), no zero-fill
// launch, the same bits from every call in either mode.  Partials are fp32 per thread over at most 8 pixels and double from
// the wave reduction on; the histogram is double from the first addition.
#include "common.hpp"
#include "taps.hpp"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int NW = NT / 64;        // waves per workgroup
constexpr int TW = 64, TH = 32;    // tile of full-resolution pixels (prep, sparsify)
constexpr int CPT = 4;             // consecutive columns per thread (one float4: af_ld_cols4 / af_st_cols4)
constexpr int RSTEP = NT / (TW / CPT);  // tile rows per pass of the workgroup: 16
constexpr int RPT = TH / RSTEP;    // rows per thread: 2
constexpr int PPT = CPT * RPT;     // pixels per thread: 8
constexpr int MAX_DIM = 16384;
constexpr int MAX_K = 32;          // thresholds per field and launch
constexpr int MAX_NB = 128;        // histogram edges
constexpr int CHUNK = NT * PPT;    // elements of one plane per histogram workgroup: 2048

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- prep ---------------------------------------------------------------------------------------------------------------
// grid (tile columns, tile rows, B); rows [B][tiles][8]: min ent_map, max ent_map, min epe, max epe, sum valid, 0, 0, 0
template <bool VEC>
__global__ __launch_bounds__(NT) void uncert_prep_kernel(const float* __restrict__ ent, const float* __restrict__ epe_map,
                                                         const float* __restrict__ valid, long valid_bstride,
                                                         float* __restrict__ ent_map, double* __restrict__ rows, float sub_w,
                                                         float add_W, float sub_h, float add_H, int h, int w, int H, int W) {
  __shared__ float red[5 * NW];
  const int b = blockIdx.z;
  const int X0 = blockIdx.x * TW + (threadIdx.x % (TW / CPT)) * CPT;
  const int Yb = blockIdx.y * TH + threadIdx.x / (TW / CPT);
  const long HW = (long)H * W, hw = (long)h * w;
  const float* e0 = ent + 2 * hw * b;
  const float* e1 = e0 + hw;
  const float* ep = epe_map + HW * b;
  const float* va = valid ? valid + valid_bstride * b : nullptr;
  float* om = ent_map + HW * b;
  const float fw = (float)w, fW = (float)W, fh = (float)h, fH = (float)H;
  const float inf = __builtin_inff();

  int xa[CPT], xb[CPT];
  float wx0[CPT], wx1[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) up_source(min(X0 + j, W - 1), w, W, fw / fW, false, xa[j], xb[j], wx0[j], wx1[j]);

  float mn_e = inf, mx_e = -inf, mn_p = inf, mx_p = -inf, sv = 0.f;
  for (int k = 0; k < RPT; ++k) {
    const int Y = Yb + k * RSTEP;
    if (Y >= H) break;
    int ya, yb;
    float wy0, wy1;
    up_source(Y, h, H, fh / fH, false, ya, yb, wy0, wy1);
    float pe[CPT], g[CPT], out[CPT];
    af_ld_cols4<VEC>(ep + (long)Y * W, X0, W, 0.f, pe);
    if (va) {
      af_ld_cols4<VEC>(va + (long)Y * W, X0, W, 0.f, g);
    } else {
#pragma unroll
      for (int j = 0; j < CPT; ++j) g[j] = X0 + j < W ? 1.f : 0.f;
    }
    const float* a0 = e0 + ya * w;
    const float* b0 = e0 + yb * w;
    const float* a1 = e1 + ya * w;
    const float* b1 = e1 + yb * w;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      // the shift BEFORE the resize, two fp32 roundings per tap in the reference's order: (x - 2 log w) + 2 log W
      const float c0 = up_blend(wx0[j], wx1[j], wy0, wy1, (a0[xa[j]] - sub_w) + add_W, (a0[xb[j]] - sub_w) + add_W,
                                (b0[xa[j]] - sub_w) + add_W, (b0[xb[j]] - sub_w) + add_W);
      const float c1 = up_blend(wx0[j], wx1[j], wy0, wy1, (a1[xa[j]] - sub_h) + add_H, (a1[xb[j]] - sub_h) + add_H,
                                (b1[xa[j]] - sub_h) + add_H, (b1[xb[j]] - sub_h) + add_H);
      out[j] = c0 + c1;
      if (X0 + j < W) {  // a column beyond W took the taps of column W - 1: drop it
        mn_e = fminf(mn_e, out[j]), mx_e = fmaxf(mx_e, out[j]);
        mn_p = fminf(mn_p, pe[j]), mx_p = fmaxf(mx_p, pe[j]);
        sv += g[j];
      }
    }
    af_st_cols4<VEC>(om + (long)Y * W, X0, W, out);
  }
  // sum valid: at most 8 values of a mask per thread in fp32, double from here on; min / max are exact in fp32
  const double dv = af_wave_sum((double)sv);
  mn_e = wave_min(mn_e), mx_e = wave_max(mx_e), mn_p = wave_min(mn_p), mx_p = wave_max(mx_p);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0 * NW + wave] = mn_e, red[1 * NW + wave] = mx_e, red[2 * NW + wave] = mn_p, red[3 * NW + wave] = mx_p;
    red[4 * NW + wave] = (float)dv;  // <= 512: exact
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int q = 0; q < NW; ++q) {
      mn_e = fminf(mn_e, red[0 * NW + q]), mx_e = fmaxf(mx_e, red[1 * NW + q]);
      mn_p = fminf(mn_p, red[2 * NW + q]), mx_p = fmaxf(mx_p, red[3 * NW + q]);
      s += (double)red[4 * NW + q];
    }
    const long tiles = (long)gridDim.x * gridDim.y;
    double* r = rows + 8 * (tiles * b + (long)blockIdx.y * gridDim.x + blockIdx.x);
    r[0] = (double)mn_e, r[1] = (double)mx_e, r[2] = (double)mn_p, r[3] = (double)mx_p, r[4] = s;
    r[5] = r[6] = r[7] = 0.0;
  }
}

// ---- sparsification sums --------------------------------------------------------------------------------------------------
// grid (tile columns, tile rows, B); rows [B][tiles][F][K][3]: sum (1-m) g, sum m g, sum err m g.  A thread keeps its 8
// pixels of err, the fields and the mask in registers and walks the thresholds, so every plane is read once per launch.
template <bool VEC, int F>
__global__ __launch_bounds__(NT) void sparsify_sums_kernel(const float* __restrict__ err, const float* __restrict__ field0,
                                                           const float* __restrict__ field1, const float* __restrict__ valid,
                                                           long valid_bstride, const double* __restrict__ thr, float alpha,
                                                           double* __restrict__ rows, int H, int W, int K) {
  __shared__ double part[NW * 2 * MAX_K * 3];
  const int b = blockIdx.z;
  const int X0 = blockIdx.x * TW + (threadIdx.x % (TW / CPT)) * CPT;
  const int Yb = blockIdx.y * TH + threadIdx.x / (TW / CPT);
  const long HW = (long)H * W;
  const float* va = valid ? valid + valid_bstride * b : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  float er[PPT], g[PPT];
  double fd[F][PPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int Y = Yb + k * RSTEP;
    float t[CPT];
    if (Y < H) {  // (not a break: the wave reductions below need every lane)
      const long o = HW * b + (long)Y * W;
      af_ld_cols4<VEC>(err + o, X0, W, 0.f, t);
#pragma unroll
      for (int j = 0; j < CPT; ++j) er[k * CPT + j] = t[j];
      af_ld_cols4<VEC>(field0 + o, X0, W, 0.f, t);
#pragma unroll
      for (int j = 0; j < CPT; ++j) fd[0][k * CPT + j] = (double)t[j];
      if (F == 2) {
        af_ld_cols4<VEC>(field1 + o, X0, W, 0.f, t);
#pragma unroll
        for (int j = 0; j < CPT; ++j) fd[F - 1][k * CPT + j] = (double)t[j];
      }
      if (va) {
        af_ld_cols4<VEC>(va + (long)Y * W, X0, W, 0.f, t);
#pragma unroll
        for (int j = 0; j < CPT; ++j) g[k * CPT + j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < CPT; ++j) g[k * CPT + j] = X0 + j < W ? 1.f : 0.f;
      }
    } else {  // a pixel outside the image: g = 0 and finite values, so it adds exactly 0 to all three sums
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        er[k * CPT + j] = 0.f, g[k * CPT + j] = 0.f;
#pragma unroll
        for (int f = 0; f < F; ++f) fd[f][k * CPT + j] = 0.0;
      }
    }
  }

#pragma unroll
  for (int f = 0; f < F; ++f) {
    const double* tf = thr + ((long)b * F + f) * K;
    for (int k = 0; k < K; ++k) {
      const double t = tf[k];
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int p = 0; p < PPT; ++p) {
        const float d = (float)(t - fd[f][p]);  // the difference in double: the tail keeps its relative accuracy
        const float a = alpha * d;
        const float m = 1.f / (1.f + expf(-a));  // expf, not __expf: accurately rounded; expf(+big) = inf gives m = 0
        const float mg = m * g[p];
        s0 += (1.f - m) * g[p];
        s1 += mg;
        s2 += er[p] * mg;
      }
      const double d0 = af_wave_sum((double)s0), d1 = af_wave_sum((double)s1), d2 = af_wave_sum((double)s2);
      if (lane == 0) {
        double* q = part + ((wave * F + f) * MAX_K + k) * 3;
        q[0] = d0, q[1] = d1, q[2] = d2;
      }
    }
  }
  __syncthreads();
  const long tiles = (long)gridDim.x * gridDim.y;
  double* r = rows + (tiles * b + (long)blockIdx.y * gridDim.x + blockIdx.x) * (long)(F * K * 3);
  for (int i = threadIdx.x; i < F * K * 3; i += NT) {
    const int f = i / (K * 3), rem = i - f * K * 3;  // rem = k * 3 + q
    double s = 0.0;
    for (int q = 0; q < NW; ++q) s += part[(q * F + f) * MAX_K * 3 + rem];
    r[i] = s;
  }
}

// ---- calibration histogram ------------------------------------------------------------------------------------------------
// grid (chunks of one plane, 2 channels, B); rows [B][2][chunks][nb + 1][3]: count, sum e, sum e^2.  Every wave keeps a
// private histogram in LDS; per element slot the wave walks the DISTINCT bins its lanes hold (the bin of the first remaining
// lane, a ballot of the lanes with that bin), reduces the masked values over the wave in the fixed butterfly order and lets
// one lane add them -- no LDS atomics, so the double sums are the same on every run.
template <bool VEC>
__global__ __launch_bounds__(NT) void calib_hist_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ ent, const double* __restrict__ edges,
                                                        double* __restrict__ rows, int C, int H, int W, int nb) {
  __shared__ double edge[MAX_NB];
  __shared__ double hist[NW * (MAX_NB + 1) * 3];
  const int c = blockIdx.y, b = blockIdx.z;
  const long HW = (long)H * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbin = nb + 1;
  for (int i = threadIdx.x; i < nb; i += NT) edge[i] = edges[i];
  for (int i = threadIdx.x; i < NW * nbin * 3; i += NT) hist[i] = 0.0;
  __syncthreads();

  const float* p = pred + (2L * b + c) * HW;
  const float* q = gt + ((long)C * b + c) * HW;
  const float* s = ent + (2L * b + c) * HW;
  const float den = c == 0 ? (float)W : (float)H;  // prediction and ground truth have one size: (p / w) * W, two roundings
  double* hw_ = hist + wave * nbin * 3;

#pragma unroll
  for (int k = 0; k < PPT / CPT; ++k) {
    const long i0 = (long)blockIdx.x * CHUNK + (long)k * (NT * CPT) + threadIdx.x * CPT;
    float pv[CPT], gv[CPT], sv[CPT];
    if (VEC) {
      const bool in = i0 < HW;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 t0 = in ? *reinterpret_cast<const float4*>(p + i0) : z;
      const float4 t1 = in ? *reinterpret_cast<const float4*>(q + i0) : z;
      const float4 t2 = in ? *reinterpret_cast<const float4*>(s + i0) : z;
      pv[0] = t0.x, pv[1] = t0.y, pv[2] = t0.z, pv[3] = t0.w;
      gv[0] = t1.x, gv[1] = t1.y, gv[2] = t1.z, gv[3] = t1.w;
      sv[0] = t2.x, sv[1] = t2.y, sv[2] = t2.z, sv[3] = t2.w;
    } else {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const bool in = i0 + j < HW;
        pv[j] = in ? p[i0 + j] : 0.f, gv[j] = in ? q[i0 + j] : 0.f, sv[j] = in ? s[i0 + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const bool in = i0 + j < HW;
      const float e = fabsf(af_div_den(pv[j], den) * den - gv[j]);
      const double sigma = (double)expf(sv[j]);
      // np.digitize(sigma, edges): the count of edges <= sigma (edges ascending; a NaN sorts past the last edge)
      int lo = 0, hi = nb;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edge[mid] <= sigma) lo = mid + 1;
        else hi = mid;
      }
      const int bin = sigma != sigma ? nb : lo;
      const double de = (double)e, de2 = de * de;  // exact: 24 x 24 bits
      unsigned long long left = __ballot(in);
      while (left) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)left) - 1);
        const int cur = __builtin_amdgcn_readlane(bin, first);
        const bool mine = in && bin == cur;
        const unsigned long long m = __ballot(mine);
        const double v1 = af_wave_sum(mine ? de : 0.0), v2 = af_wave_sum(mine ? de2 : 0.0);
        if (lane == first) {
          double* hb = hw_ + cur * 3;
          hb[0] += (double)__popcll(m), hb[1] += v1, hb[2] += v2;
        }
        left &= ~m;
      }
    }
  }
  __syncthreads();
  double* r = rows + ((2L * b + c) * gridDim.x + blockIdx.x) * (long)(nbin * 3);
  for (int i = threadIdx.x; i < nbin * 3; i += NT) {
    double t = 0.0;
    for (int w = 0; w < NW; ++w) t += hist[w * nbin * 3 + i];
    r[i] = t;
  }
}

}  // namespace

extern "C" int arflow_uncert_rows(int H, int W) {
  AF_REQUIRE(H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  return af_cdiv(W, TW) * af_cdiv(H, TH);
}

extern "C" int arflow_uncert_prep(const float* ent, const float* epe_map, const float* valid, long valid_bstride,
                                  float* ent_map, double* rows, float sub_w, float add_W, float sub_h, float add_H, int B,
                                  int h, int w, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(ent);
  AF_REQUIRE_PTR(epe_map);
  AF_REQUIRE_PTR(ent_map);
  AF_REQUIRE_PTR(rows);
  AF_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(B <= 65535 && h <= MAX_DIM && w <= MAX_DIM && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  AF_REQUIRE(valid == nullptr || valid_bstride >= (long)H * W, ARFLOW_ESHAPE);
  const dim3 grid(af_cdiv(W, TW), af_cdiv(H, TH), B);
  const bool vec = W % 4 == 0 && af_aligned16(epe_map) && af_aligned16(ent_map) && af_aligned16(valid) &&
                   (valid == nullptr || valid_bstride % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(uncert_prep_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, ent, epe_map, valid, valid_bstride,
                       ent_map, rows, sub_w, add_W, sub_h, add_H, h, w, H, W);
  else
    hipLaunchKernelGGL(uncert_prep_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, ent, epe_map, valid, valid_bstride,
                       ent_map, rows, sub_w, add_W, sub_h, add_H, h, w, H, W);
  return af_launch_status();
}

extern "C" int arflow_sparsify_sums(const float* err, const float* field0, const float* field1, const float* valid,
                                    long valid_bstride, const double* thr, float alpha, double* rows, int B, int H, int W,
                                    int K, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(err);
  AF_REQUIRE_PTR(field0);
  AF_REQUIRE_PTR(thr);
  AF_REQUIRE_PTR(rows);
  AF_REQUIRE(B >= 1 && H >= 1 && W >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(B <= 65535 && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  AF_REQUIRE(valid == nullptr || valid_bstride >= (long)H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(K >= 1 && K <= MAX_K, ARFLOW_EPARAM);
  const dim3 grid(af_cdiv(W, TW), af_cdiv(H, TH), B);
  const bool vec = W % 4 == 0 && af_aligned16(err) && af_aligned16(field0) && af_aligned16(field1) && af_aligned16(valid) &&
                   (valid == nullptr || valid_bstride % 4 == 0);
#define AF_SPARSIFY(VEC, F)                                                                                              \
  hipLaunchKernelGGL((sparsify_sums_kernel<VEC, F>), grid, dim3(NT), 0, (hipStream_t)stream, err, field0, field1, valid, \
                     valid_bstride, thr, alpha, rows, H, W, K)
  if (field1 != nullptr) {
    if (vec) AF_SPARSIFY(true, 2);
    else AF_SPARSIFY(false, 2);
  } else {
    if (vec) AF_SPARSIFY(true, 1);
    else AF_SPARSIFY(false, 1);
  }
#undef AF_SPARSIFY
  return af_launch_status();
}

extern "C" int arflow_calib_rows(int H, int W) {
  AF_REQUIRE(H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  return 2 * af_cdiv((long)H * W, CHUNK);
}

extern "C" int arflow_calib_hist(const float* pred, const float* gt, const float* ent, const double* edges, double* rows,
                                 int B, int C, int H, int W, int nb, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(pred);
  AF_REQUIRE_PTR(gt);
  AF_REQUIRE_PTR(ent);
  AF_REQUIRE_PTR(edges);
  AF_REQUIRE_PTR(rows);
  AF_REQUIRE(B >= 1 && H >= 1 && W >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(B <= 65535 && H <= MAX_DIM && W <= MAX_DIM, ARFLOW_ESHAPE);
  AF_REQUIRE(C == 2 || C == 4, ARFLOW_EPARAM);
  AF_REQUIRE(nb >= 1 && nb <= MAX_NB, ARFLOW_EPARAM);
  const long HW = (long)H * W;
  const dim3 grid(af_cdiv(HW, CHUNK), 2, B);
  // float4 pieces of the flattened planes: every plane starts 16-byte aligned when H * W % 4 == 0
  const bool vec = HW % 4 == 0 && af_aligned16(pred) && af_aligned16(gt) && af_aligned16(ent);
  if (vec)
    hipLaunchKernelGGL(calib_hist_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, pred, gt, ent, edges, rows, C, H, W,
                       nb);
  else
    hipLaunchKernelGGL(calib_hist_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, pred, gt, ent, edges, rows, C, H, W,
                       nb);
  return af_launch_status();
}
