// The dense flow estimator's elementwise work (models/pwclite.py:48-66: five times x = cat([conv(x), x], 1), then the
// head) for gfx950.  MIOpen keeps the convolutions; what surrounds them was, per layer, a bias/LeakyReLU pass in place
// and a torch.cat forward, and a slice copy, the LeakyReLU-derivative pass and a strided add over the whole remaining
// suffix of the concatenation backward.  Two kernels replace them:
//   dense_cat_fwd       writes lrelu(y + bias) and the layer's input straight into their slots of the next tensor;
//   dense_grad_gather   forms the gradient of one layer's activation from the slices of every tensor that holds a
//                       part of it -- each element of each data gradient is read once, where it is consumed -- applies
//                       the LeakyReLU derivative from the saved activation, and leaves the bias gradient as
//                       per-workgroup partial rows (no zero-fill launch, no atomics).
// Both stream at HBM speed; the arithmetic and its order are those of the composed tensor expression (the Makefile
// builds with -ffp-contract=off), so MIOpen's backward kernels receive bit-identical inputs.
#include "common.hpp"

namespace {
constexpr int NT = 256, EPT = 16;  // as act.hip: 4 float4 per thread, grid (chunks of a plane, channel, sample)

// out[b, c, :] = c < oc ? lrelu(y[b, c, :] + bias[c]) : x[b, c - oc, :];  out: [B, oc + C, HW] packed.
// The activation arithmetic is bias_act_fwd_kernel's (v += b; v > 0 ? v : v * slope).
__global__ __launch_bounds__(NT) void dense_cat_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                           const float* __restrict__ x, float* __restrict__ out, int oc,
                                                           int C, long HW, float slope) {
  const int c = blockIdx.y;
  const bool is_act = c < oc;
  const float* src = is_act ? y + ((long)blockIdx.z * oc + c) * HW : x + ((long)blockIdx.z * C + (c - oc)) * HW;
  float* dst = out + ((long)blockIdx.z * (oc + C) + c) * HW;
  const float bv = (is_act && bias) ? bias[c] : 0.f;
  auto f = [&](float v) {
    if (!is_act) return v;
    v += bv;
    return v > 0.f ? v : v * slope;
  };
  if ((HW & 3) == 0) {
    const long n4 = HW / 4;
    float4 v[EPT / 4];
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const long i = ((long)blockIdx.x * (EPT / 4) + k) * NT + threadIdx.x;
      if (i < n4) v[k] = reinterpret_cast<const float4*>(src)[i];
    }
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const long i = ((long)blockIdx.x * (EPT / 4) + k) * NT + threadIdx.x;
      if (i < n4) reinterpret_cast<float4*>(dst)[i] = make_float4(f(v[k].x), f(v[k].y), f(v[k].z), f(v[k].w));
    }
  } else {
    for (long i = (long)blockIdx.x * NT * EPT + threadIdx.x; i < min(HW, ((long)blockIdx.x + 1) * NT * EPT); i += NT)
      dst[i] = f(src[i]);
  }
}

struct GatherArgs {  // by value in the kernel arguments (as LevelBwdArgs travels): no device-side table to fill
  const float* ptr[ARFLOW_DENSE_MAX_SRC];
  long bstride[ARFLOW_DENSE_MAX_SRC];
  const float* scale[ARFLOW_DENSE_MAX_SRC];
};

// gy[b, c, :] = d(act[b, c, :]) * (s_0 (+) s_1 (+) ...) with acc = s_0 * scale_0[b]; acc = s_1 * scale_1[b] + acc; ...
// (innermost first: the nesting autograd's own accumulation has), d = act > 0 ? 1 : slope, or 1 without `act`.
// The workgroup's sum of gy goes to row (b * gridDim.x + blockIdx.x) of gbias_rows ([rows][oc]).
// N sources as a template parameter: the N loads of every float4 are independent and issued back to back.
template <int N, bool VEC>
__global__ __launch_bounds__(NT) void dense_grad_gather_kernel(GatherArgs a, const float* __restrict__ act, long act_bs,
                                                               float* __restrict__ gy, float* __restrict__ gbias_rows,
                                                               int oc, long HW, float slope) {
  __shared__ float red[NT / 64];
  const int c = blockIdx.y, b = blockIdx.z;
  const float* sp[N];
  float sc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    sp[j] = a.ptr[j] + (long)b * a.bstride[j] + (long)c * HW;
    sc[j] = a.scale[j] ? a.scale[j][b] : 1.f;
  }
  const float* ap = act ? act + (long)b * act_bs + (long)c * HW : nullptr;
  float* gp = gy + ((long)b * oc + c) * HW;
  float s[1] = {0.f};
  // x * 1.0f is x for every float, so the unscaled sources keep their bits
  auto scaled = [&](float v, int j) { return a.scale[j] ? v * sc[j] : v; };
  auto d = [&](float g, float v) { return v > 0.f ? g : g * slope; };
  if (VEC) {
    const long n4 = HW / 4;
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const long i = ((long)blockIdx.x * (EPT / 4) + k) * NT + threadIdx.x;
      if (i < n4) {
        float4 v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = reinterpret_cast<const float4*>(sp[j])[i];
        float4 r = make_float4(scaled(v[0].x, 0), scaled(v[0].y, 0), scaled(v[0].z, 0), scaled(v[0].w, 0));
#pragma unroll
        for (int j = 1; j < N; ++j) {
          r.x = scaled(v[j].x, j) + r.x;
          r.y = scaled(v[j].y, j) + r.y;
          r.z = scaled(v[j].z, j) + r.z;
          r.w = scaled(v[j].w, j) + r.w;
        }
        if (ap) {
          const float4 y = reinterpret_cast<const float4*>(ap)[i];
          r = make_float4(d(r.x, y.x), d(r.y, y.y), d(r.z, y.z), d(r.w, y.w));
        }
        reinterpret_cast<float4*>(gp)[i] = r;
        s[0] += (r.x + r.y) + (r.z + r.w);
      }
    }
  } else {
    for (long i = (long)blockIdx.x * NT * EPT + threadIdx.x; i < min(HW, ((long)blockIdx.x + 1) * NT * EPT); i += NT) {
      float r = scaled(sp[0][i], 0);
#pragma unroll
      for (int j = 1; j < N; ++j) r = scaled(sp[j][i], j) + r;
      if (ap) r = d(r, ap[i]);
      gp[i] = r;
      s[0] += r;
    }
  }
  if (gbias_rows) {
    af_block_sum<1>(s, red);
    if (threadIdx.x == 0) gbias_rows[((long)b * gridDim.x + blockIdx.x) * oc + c] = s[0];
  }
}

template <int N>
void launch_gather(const GatherArgs& a, bool vec, dim3 grid, hipStream_t st, const float* act, long act_bs, float* gy,
                   float* gbias_rows, int oc, long HW, float slope) {
  if (vec)
    hipLaunchKernelGGL((dense_grad_gather_kernel<N, true>), grid, dim3(NT), 0, st, a, act, act_bs, gy, gbias_rows, oc, HW, slope);
  else
    hipLaunchKernelGGL((dense_grad_gather_kernel<N, false>), grid, dim3(NT), 0, st, a, act, act_bs, gy, gbias_rows, oc, HW, slope);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" int arflow_dense_cat_fwd(const float* y, const float* bias, const float* x, float* out, int B, int oc, int C,
                                    long HW, float negative_slope, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(y);
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(out);
  AF_REQUIRE(B > 0 && oc > 0 && C > 0 && HW > 0 && B <= 65535 && (long)oc + C <= 65535, ARFLOW_ESHAPE);
  // packed planes of HW floats: with HW % 4 == 0 every plane starts 16-byte aligned iff the base pointers do
  AF_REQUIRE((HW & 3) != 0 || (aligned16(y) && aligned16(x) && aligned16(out)), ARFLOW_EPARAM);
  hipLaunchKernelGGL(dense_cat_fwd_kernel, dim3(af_cdiv(HW, NT * EPT), oc + C, B), dim3(NT), 0, (hipStream_t)stream, y, bias, x,
                     out, oc, C, HW, negative_slope);
  return af_launch_status();
}

extern "C" int arflow_dense_gbias_rows(int B, long HW) {
  return (B > 0 && HW > 0 && B <= 65535) ? B * af_cdiv(HW, NT * EPT) : ARFLOW_ESHAPE;
}

extern "C" int arflow_dense_grad_gather(const arflow_dense_src* srcs, int n_src, const float* act, long act_bs, float* gy,
                                        float* gbias_rows, int B, int oc, long HW, float negative_slope,
                                        arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(srcs);
  AF_REQUIRE_PTR(gy);
  AF_REQUIRE(n_src >= 1 && n_src <= ARFLOW_DENSE_MAX_SRC, ARFLOW_EPARAM);
  AF_REQUIRE(B > 0 && oc > 0 && HW > 0 && B <= 65535 && oc <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(act == nullptr || act_bs >= (long)oc * HW, ARFLOW_EPARAM);
  GatherArgs a = {};
  bool vec = (HW & 3) == 0 && aligned16(gy) && (act == nullptr || (aligned16(act) && (act_bs & 3) == 0));
  for (int j = 0; j < n_src; ++j) {
    AF_REQUIRE_PTR(srcs[j].ptr);
    AF_REQUIRE(srcs[j].bstride >= (long)oc * HW, ARFLOW_EPARAM);
    a.ptr[j] = srcs[j].ptr, a.bstride[j] = srcs[j].bstride, a.scale[j] = srcs[j].scale;
    vec = vec && aligned16(srcs[j].ptr) && (srcs[j].bstride & 3) == 0;
  }
  const dim3 grid(af_cdiv(HW, NT * EPT), oc, B);
  hipStream_t st = (hipStream_t)stream;
  switch (n_src) {
#define AF_GATHER_CASE(N) \
  case N:                 \
    launch_gather<N>(a, vec, grid, st, act, act_bs, gy, gbias_rows, oc, HW, negative_slope); \
    break;
    AF_GATHER_CASE(1)
    AF_GATHER_CASE(2)
    AF_GATHER_CASE(3)
    AF_GATHER_CASE(4)
    AF_GATHER_CASE(5)
    AF_GATHER_CASE(6)
    AF_GATHER_CASE(7)
    AF_GATHER_CASE(8)
#undef AF_GATHER_CASE
  }
  return af_launch_status();
}
