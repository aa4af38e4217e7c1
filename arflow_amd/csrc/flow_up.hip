// Flow upsample with a gather adjoint: F.interpolate(flow * s, scale_factor=s, mode='bilinear') for
// s = 2, 4 -- how the reference models bring a flow to the next pyramid level or to full resolution (models/pwclite.py:
// 54,66,92,104; models/pwclite_uflow.py:104,124; utils/uflow_utils.py:163-180 upsample(is_flow)).  ATen's backward of that
// call scatters with float atomics; here the adjoint is a gather with a fixed order of additions, so the models' flow path
// is reproducible in deterministic mode.  (The x2 case inside the fused level keeps its own kernels: up2_source /
// up2_bwd_kernel, warp.hip -- this file is their generalisation to a factor argument; the index arithmetic is shared.)
#include "common.hpp"
#include "taps.hpp"

namespace {
// Source rows / weights: up_source (taps.hpp) with rs = 1 / factor (exact) -- the same device code as the level's x2 case.
// one thread per fine pixel; planes = 2 B
__global__ __launch_bounds__(256) void flow_up_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, int planes,
                                                          int h, int w, int factor, int align) {
  const int H = h * factor, W = w * factor;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)planes * H * W) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const long pl = idx / ((long)W * H);
  const float rs = 1.f / (float)factor, f = (float)factor;
  int xa, xb, ya, yb;
  float wx0, wx1, wy0, wy1;
  up_source(x, w, W, rs, align != 0, xa, xb, wx0, wx1);
  up_source(y, h, H, rs, align != 0, ya, yb, wy0, wy1);
  const float* s = in + pl * h * w;
  const float a00 = s[ya * w + xa], a01 = s[ya * w + xb], a10 = s[yb * w + xa], a11 = s[yb * w + xb];
  // interpolate(f * v) = f * interpolate(v) exactly in fp32: a power-of-two scale commutes with every rounding
  out[idx] = f * up_blend(wx0, wx1, wy0, wy1, a00, a01, a10, a11);
}

// Adjoint: one thread per coarse cell (i, j) over the run of fine rows / columns fine_run (taps.hpp) gives; rows ascending,
// columns ascending inside a row: a fixed order.
__global__ __launch_bounds__(256) void flow_up_bwd_kernel(const float* __restrict__ gfine, float* __restrict__ gcoarse,
                                                          int planes, int h, int w, int factor, int align) {
  const int H = h * factor, W = w * factor;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)planes * h * w) return;
  const int j = (int)(idx % w), i = (int)((idx / w) % h);
  const long pl = idx / ((long)w * h);
  const float* g = gfine + pl * H * W;
  const float rs = 1.f / (float)factor;
  int ylo, yhi, xlo, xhi;
  fine_run(i, h, H, factor, align != 0, ylo, yhi);
  fine_run(j, w, W, factor, align != 0, xlo, xhi);
  float acc = 0.f;
  for (int y = ylo; y <= yhi; ++y) {
    int a0, a1;
    float l0, l1;
    up_source(y, h, H, rs, align != 0, a0, a1, l0, l1);
    const float wy = (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
    float row = 0.f;
    for (int x = xlo; x <= xhi; ++x) {
      up_source(x, w, W, rs, align != 0, a0, a1, l0, l1);
      const float wx = (a0 == j ? l0 : 0.f) + (a1 == j ? l1 : 0.f);
      row = fmaf(wx, g[(long)y * W + x], row);
    }
    acc = fmaf(wy, row, acc);
  }
  gcoarse[idx] = (float)factor * acc;
}

int flow_up_check(const void* a, const void* b, int B, int h, int w, int factor) {
  AF_REQUIRE_PTR(a);
  AF_REQUIRE_PTR(b);
  AF_REQUIRE(B > 0 && h > 0 && w > 0 && B <= 65535 && h <= 16384 && w <= 16384, ARFLOW_ESHAPE);
  AF_REQUIRE(factor == 2 || factor == 4, ARFLOW_EPARAM);
  return ARFLOW_OK;
}
}  // namespace

extern "C" int arflow_flow_up_fwd(const float* flow, float* out, int B, int h, int w, int factor, int align_corners,
                                  arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = flow_up_check(flow, out, B, h, w, factor);
  if (rc != ARFLOW_OK) return rc;
  const long n = (long)B * 2 * h * w * factor * factor;
  hipLaunchKernelGGL(flow_up_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flow, out, B * 2,
                     h, w, factor, align_corners);
  return af_launch_status();
}

extern "C" int arflow_flow_up_bwd(const float* gfine, float* gcoarse, int B, int h, int w, int factor, int align_corners,
                                  arflow_stream_t stream) {
  af_clear_stale_error();
  const int rc = flow_up_check(gfine, gcoarse, B, h, w, factor);
  if (rc != ARFLOW_OK) return rc;
  const long n = (long)B * 2 * h * w;
  hipLaunchKernelGGL(flow_up_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gfine, gcoarse,
                     B * 2, h, w, factor, align_corners);
  return af_launch_status();
}
