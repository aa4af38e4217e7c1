// MseLoss: losses/mse_loss.py:9-148 -- the squared error of S reparameterised samples of the level-2
// output against the resized ground-truth flow, the sum of the log-diagonal and the off-diagonal regulariser -- in ONE call
// forward and one backward, and the standalone resize_flow (utils/flow_utils.py:110-118).
//   net [B][C][h][w]: mean 0:2, log_diag 2:4, (given-z mode) left 4:6 without its last column, over 6:8 without its last row
//   target [B][2][H][W];  ez [S B][2][h][w], sample n = s B + b:  the noise eps (sampling modes) or the samples z (given-z mode)
//   mode 0 (covariance):  z = mean + RN(expf(log_diag) eps)      mode 1 (inv_cov):  z = mean + RN(expf(-log_diag) eps)
//   mode 2 (given z):     z is read (the 4-neighbour samplers of triag_solve.py wrote it)
//   forward:  gt = resize_flow(target) (resize_dev.hpp), r = z - gt in fp32, then in float64 from that point on
//             sums = { sum r^2,  sum log_diag,  sum left^2,  sum over^2 }           (the last two 0 in the sampling modes)
//   backward: c = (float)(2 gsums[0]), ge = (float)gsums[1], cl = (float)(2 gsums[2]), co = (float)(2 gsums[3]);  gz = c r
//             sampling:  gmean = sum_s gz,  glog_diag = sum_s gz (+- std eps) + ge,  channels 4.. zero
//             given z:   gz stored [S B][2][h][w];  gnet: 0:2 zero, 2:4 ge, 4:6 cl left, 6:8 co over (zero in the column / row
//                        the slices leave out), channels 8.. zero
// One lane takes one pixel (b, y, x) and both channels, lanes along x; it forms gt once, loads mean and log_diag once and
// loops over the samples.  Sums: per lane in (sample, channel) order, over the workgroup by af_block_sum_f64 (common.hpp), ONE
// row of four float64 partials per workgroup in `work`; a second one-wave launch of the same call folds the rows lane-strided in
// index order and by butterfly.  No atomics, no zero-fill: the same code and bits in normal and deterministic mode.  Every
// element of every output is stored.
#include "common.hpp"
#include "resize_dev.hpp"

namespace {

constexpr int MS_NT = 256;
constexpr int MS_COV = 0, MS_INV = 1, MS_GIVEN = 2;
constexpr long MS_MAX_PLANE = 0x3fffffffL;

struct MsArgs {
  const float* net;
  const float* tgt;
  const float* ez;
  long net_bs, tgt_bs, ez_bs;
  int B, S, C, h, w, H, W, mode, align;
};

// the standard deviation, stated once: forward and backward must agree bit for bit
__device__ __forceinline__ float ms_std(float log_diag, int mode) { return expf(mode == MS_INV ? -log_diag : log_diag); }

__global__ __launch_bounds__(MS_NT) void mse_fwd_kernel(const MsArgs a, double* __restrict__ work) {
  __shared__ double part[4 * (MS_NT / AF_WAVE)];
  const long hw = (long)a.h * a.w;
  const long p = (long)blockIdx.x * MS_NT + threadIdx.x;
  const int b = blockIdx.y;
  double acc[4] = {0., 0., 0., 0.};
  if (p < hw) {
    const int y = (int)(p / a.w), x = (int)(p % a.w);
    float g0, g1;
    rf_resize_flow(a.tgt + b * a.tgt_bs, a.H, a.W, a.h, a.w, y, x, a.align, g0, g1);
    const float* nb = a.net + b * a.net_bs + p;
    const float ld0 = nb[2 * hw], ld1 = nb[3 * hw];
    acc[1] = (double)ld0 + (double)ld1;
    if (a.mode != MS_GIVEN) {
      const float m0 = nb[0], m1 = nb[hw];
      const float s0 = ms_std(ld0, a.mode), s1 = ms_std(ld1, a.mode);
      for (int s = 0; s < a.S; ++s) {
        const float* e = a.ez + ((long)s * a.B + b) * a.ez_bs + p;
        const float t0 = s0 * e[0], t1 = s1 * e[hw];
        const float z0 = m0 + t0, z1 = m1 + t1;
        const float r0 = z0 - g0, r1 = z1 - g1;
        acc[0] += (double)r0 * (double)r0;
        acc[0] += (double)r1 * (double)r1;
      }
    } else {
      for (int s = 0; s < a.S; ++s) {
        const float* z = a.ez + ((long)s * a.B + b) * a.ez_bs + p;
        const float r0 = z[0] - g0, r1 = z[hw] - g1;
        acc[0] += (double)r0 * (double)r0;
        acc[0] += (double)r1 * (double)r1;
      }
      if (x < a.w - 1) {
        const double l0 = (double)nb[4 * hw], l1 = (double)nb[5 * hw];
        acc[2] = l0 * l0 + l1 * l1;
      }
      if (y < a.h - 1) {
        const double o0 = (double)nb[6 * hw], o1 = (double)nb[7 * hw];
        acc[3] = o0 * o0 + o1 * o1;
      }
    }
  }
  af_block_sum_f64<4, MS_NT>(acc, part);
  if (threadIdx.x == 0) {
    double* row = work + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) row[k] = acc[k];
  }
}

// one wave: sums[k] = the n partial rows in index order, lane-strided, then by butterfly
__global__ __launch_bounds__(AF_WAVE) void mse_fold_kernel(const double* __restrict__ work, long n, double* __restrict__ sums) {
  double acc[4] = {0., 0., 0., 0.};
  for (long j = threadIdx.x; j < n; j += AF_WAVE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += work[j * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = af_wave_sum(acc[k]);
    if (threadIdx.x == 0) sums[k] = v;
  }
}

__global__ __launch_bounds__(MS_NT) void mse_bwd_kernel(const MsArgs a, const double* __restrict__ gsums,
                                                        float* __restrict__ gnet, long gnet_bs, float* __restrict__ gz,
                                                        long gz_bs) {
  const long hw = (long)a.h * a.w;
  const long p = (long)blockIdx.x * MS_NT + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= hw) return;
  const float c = (float)(2.0 * gsums[0]), ge = (float)gsums[1];
  const int y = (int)(p / a.w), x = (int)(p % a.w);
  float g0, g1;
  rf_resize_flow(a.tgt + b * a.tgt_bs, a.H, a.W, a.h, a.w, y, x, a.align, g0, g1);
  const float* nb = a.net + b * a.net_bs + p;
  float* gb = gnet + b * gnet_bs + p;
  int first_zero;
  if (a.mode != MS_GIVEN) {
    const float ld0 = nb[2 * hw], ld1 = nb[3 * hw];
    const float m0 = nb[0], m1 = nb[hw];
    const float s0 = ms_std(ld0, a.mode), s1 = ms_std(ld1, a.mode);
    float gm0 = 0.f, gm1 = 0.f, gl0 = 0.f, gl1 = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const float* e = a.ez + ((long)s * a.B + b) * a.ez_bs + p;
      const float t0 = s0 * e[0], t1 = s1 * e[hw];
      const float z0 = m0 + t0, z1 = m1 + t1;
      const float gz0 = c * (z0 - g0), gz1 = c * (z1 - g1);
      gm0 += gz0, gm1 += gz1;
      gl0 += gz0 * (a.mode == MS_INV ? -t0 : t0);
      gl1 += gz1 * (a.mode == MS_INV ? -t1 : t1);
    }
    gb[0] = gm0, gb[hw] = gm1;
    gb[2 * hw] = gl0 + ge, gb[3 * hw] = gl1 + ge;
    first_zero = 4;
  } else {
    for (int s = 0; s < a.S; ++s) {
      const long n = (long)s * a.B + b;
      const float* z = a.ez + n * a.ez_bs + p;
      float* g = gz + n * gz_bs + p;
      g[0] = c * (z[0] - g0);
      g[hw] = c * (z[hw] - g1);
    }
    const float cl = (float)(2.0 * gsums[2]), co = (float)(2.0 * gsums[3]);
    gb[0] = 0.f, gb[hw] = 0.f;
    gb[2 * hw] = ge, gb[3 * hw] = ge;
    const bool in_l = x < a.w - 1, in_o = y < a.h - 1;
    gb[4 * hw] = in_l ? cl * nb[4 * hw] : 0.f;
    gb[5 * hw] = in_l ? cl * nb[5 * hw] : 0.f;
    gb[6 * hw] = in_o ? co * nb[6 * hw] : 0.f;
    gb[7 * hw] = in_o ? co * nb[7 * hw] : 0.f;
    first_zero = 8;
  }
  for (int ch = first_zero; ch < a.C; ++ch) gb[ch * hw] = 0.f;
}

__global__ __launch_bounds__(MS_NT) void resize_flow_kernel(const float* __restrict__ flow, long flow_bs, int H, int W,
                                                            float* __restrict__ out, long out_bs, int h, int w, int align) {
  const long hw = (long)h * w;
  const long p = (long)blockIdx.x * MS_NT + threadIdx.x;
  if (p >= hw) return;
  const int b = blockIdx.y;
  float g0, g1;
  rf_resize_flow(flow + b * flow_bs, H, W, h, w, (int)(p / w), (int)(p % w), align, g0, g1);
  float* o = out + b * out_bs + p;
  o[0] = g0, o[hw] = g1;
}

// [p, p + n floats) of two tensors share a byte
inline bool ms_overlap(const void* p, long n, size_t size_p, const void* q, long m, size_t size_q) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + (uintptr_t)n * size_p, b0 = (uintptr_t)q, b1 = b0 + (uintptr_t)m * size_q;
  return a0 < b1 && b0 < a1;
}
inline long ms_extent(long items, long bs, long item) { return (items - 1) * bs + item; }

// the arguments the forward and the backward share -> the kernel's argument block
inline int ms_check(const float* net, long net_bs, int C, const float* target, long target_bs, int H, int W, const float* ez,
                    long ez_bs, int B, int S, int h, int w, int mode, int align, MsArgs& a) {
  AF_REQUIRE_PTR(net);
  AF_REQUIRE_PTR(target);
  AF_REQUIRE_PTR(ez);
  AF_REQUIRE(mode == MS_COV || mode == MS_INV || mode == MS_GIVEN, ARFLOW_EPARAM);
  AF_REQUIRE(align == 0 || align == 1, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && S >= 1 && (long)S * B <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1 && (long)h * w <= MS_MAX_PLANE && (long)H * W <= MS_MAX_PLANE, ARFLOW_ESHAPE);
  AF_REQUIRE(mode == MS_GIVEN ? (C >= 8 && h >= 2 && w >= 2) : C >= 4, ARFLOW_ESHAPE);
  const long hw = (long)h * w;
  AF_REQUIRE(B == 1 || (net_bs >= C * hw && target_bs >= 2L * H * W), ARFLOW_ESHAPE);
  AF_REQUIRE((long)S * B == 1 || ez_bs >= 2 * hw, ARFLOW_ESHAPE);
  a.net = net, a.tgt = target, a.ez = ez;
  a.net_bs = net_bs, a.tgt_bs = target_bs, a.ez_bs = ez_bs;
  a.B = B, a.S = S, a.C = C, a.h = h, a.w = w, a.H = H, a.W = W, a.mode = mode, a.align = align;
  return ARFLOW_OK;
}

// an output [p, p + n) against the three inputs
inline bool ms_hits_input(const MsArgs& a, const void* p, long n, size_t size) {
  const long hw = (long)a.h * a.w;
  return ms_overlap(p, n, size, a.net, ms_extent(a.B, a.net_bs, a.C * hw), 4) ||
         ms_overlap(p, n, size, a.tgt, ms_extent(a.B, a.tgt_bs, 2L * a.H * a.W), 4) ||
         ms_overlap(p, n, size, a.ez, ms_extent((long)a.S * a.B, a.ez_bs, 2 * hw), 4);
}

inline long ms_blocks(int h, int w) { return ((long)h * w + MS_NT - 1) / MS_NT; }

}  // namespace

extern "C" long arflow_mse_work_size(int B, int h, int w) {
  AF_REQUIRE(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (long)h * w <= MS_MAX_PLANE, ARFLOW_ESHAPE);
  return 4 * ms_blocks(h, w) * B;
}

extern "C" int arflow_mse_fwd(const float* net, long net_bs, int C, const float* target, long target_bs, int H, int W,
                              const float* ez, long ez_bs, int B, int S, int h, int w, int mode, int align_corners,
                              double* work, double* sums, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(work);
  AF_REQUIRE_PTR(sums);
  MsArgs a = {};
  const int rc = ms_check(net, net_bs, C, target, target_bs, H, W, ez, ez_bs, B, S, h, w, mode, align_corners, a);
  if (rc != ARFLOW_OK) return rc;
  const long nbx = ms_blocks(h, w), rows = nbx * B;
  AF_REQUIRE(!ms_hits_input(a, work, 4 * rows, 8) && !ms_hits_input(a, sums, 4, 8) && !ms_overlap(work, 4 * rows, 8, sums, 4, 8),
             ARFLOW_EPARAM);
  hipLaunchKernelGGL(mse_fwd_kernel, dim3((unsigned)nbx, (unsigned)B), dim3(MS_NT), 0, (hipStream_t)stream, a, work);
  AF_LAUNCH_CHECK();
  hipLaunchKernelGGL(mse_fold_kernel, dim3(1), dim3(AF_WAVE), 0, (hipStream_t)stream, work, rows, sums);
  return af_launch_status();
}

extern "C" int arflow_mse_bwd(const float* net, long net_bs, int C, const float* target, long target_bs, int H, int W,
                              const float* ez, long ez_bs, const double* gsums, float* gnet, long gnet_bs, float* gz,
                              long gz_bs, int B, int S, int h, int w, int mode, int align_corners, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(gsums);
  AF_REQUIRE_PTR(gnet);
  MsArgs a = {};
  const int rc = ms_check(net, net_bs, C, target, target_bs, H, W, ez, ez_bs, B, S, h, w, mode, align_corners, a);
  if (rc != ARFLOW_OK) return rc;
  const long hw = (long)h * w;
  AF_REQUIRE(B == 1 || gnet_bs >= C * hw, ARFLOW_ESHAPE);
  const long gnet_n = ms_extent(B, gnet_bs, C * hw);
  AF_REQUIRE(!ms_hits_input(a, gnet, gnet_n, 4) && !ms_overlap(gnet, gnet_n, 4, gsums, 4, 8), ARFLOW_EPARAM);
  if (mode == MS_GIVEN) {
    AF_REQUIRE_PTR(gz);
    AF_REQUIRE((long)S * B == 1 || gz_bs >= 2 * hw, ARFLOW_ESHAPE);
    const long gz_n = ms_extent((long)S * B, gz_bs, 2 * hw);
    AF_REQUIRE(!ms_hits_input(a, gz, gz_n, 4) && !ms_overlap(gz, gz_n, 4, gsums, 4, 8) && !ms_overlap(gz, gz_n, 4, gnet, gnet_n, 4),
               ARFLOW_EPARAM);
  }
  hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)ms_blocks(h, w), (unsigned)B), dim3(MS_NT), 0, (hipStream_t)stream, a,
                     gsums, gnet, gnet_bs, gz, gz_bs);
  return af_launch_status();
}

extern "C" int arflow_resize_flow(const float* flow, long flow_bs, int H, int W, float* out, long out_bs, int B, int h, int w,
                                  int align_corners, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(out);
  AF_REQUIRE(align_corners == 0 || align_corners == 1, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && B <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1 && (long)h * w <= MS_MAX_PLANE && (long)H * W <= MS_MAX_PLANE, ARFLOW_ESHAPE);
  const long hw = (long)h * w;
  AF_REQUIRE(B == 1 || (flow_bs >= 2L * H * W && out_bs >= 2 * hw), ARFLOW_ESHAPE);
  AF_REQUIRE(!ms_overlap(out, ms_extent(B, out_bs, 2 * hw), 4, flow, ms_extent(B, flow_bs, 2L * H * W), 4), ARFLOW_EPARAM);
  hipLaunchKernelGGL(resize_flow_kernel, dim3((unsigned)ms_blocks(h, w), (unsigned)B), dim3(MS_NT), 0, (hipStream_t)stream, flow,
                     flow_bs, H, W, out, out_bs, h, w, align_corners);
  return af_launch_status();
}
