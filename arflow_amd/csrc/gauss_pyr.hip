// The diagonal Gaussian sampler of ElboLoss over a whole pyramid: losses/elbo_loss.py:17-27,90-91,
// 117-124 -- per scale and direction one reparameterised sample and the sum of the log-variances -- for all n <= 6 scales in
// ONE launch, and its adjoint in one launch.
//   net_i [B,8,h_i,w_i]: mean_fw 0:2, logvar_fw 2:4, mean_bw 4:6, logvar_bw 6:8 (the trainer's cat(fw, bw))
//   eps_i [B,4,h_i,w_i]: forward noise 0:2, backward noise 2:4;   z_i [B,4,h_i,w_i]: forward sample 0:2, backward sample 2:4
//   forward:   z = mean + RN(expf(logvar / 2) * eps)           (-ffp-contract=off: the product is rounded, then the sum)
//              ent[i,d] = sum_{b,c,p} logvar_d                  float64 from the load on
//   backward:  gmean = gz;   glogvar = gz * (0.5f * expf(logvar / 2) * eps) + (float)gent[i,d]
// The two mean planes of one (b, d) are 2 h w consecutive floats, and so are its two log-variance, noise and sample planes: a
// "row".  A workgroup takes CHUNK consecutive elements of one row of one scale; it finds the scale from the prefix table of
// chunk counts that travels with the pointers in the kernel argument (by value: no device-side table, no copy).  Entropy: every
// lane adds its terms in element order, the workgroup adds them in the order of af_block_sum_f64 (common.hpp) and stores
// ONE float64 partial at work[its index]; the fold kernel (one wave per (i, d)) adds the partials lane-strided in index order
// and by butterfly.  No atomics: the same code and bits in normal and deterministic mode.  Every element of every output is
// stored (ent by the fold, z / gnet by the map).
#include "common.hpp"

namespace {

constexpr int GP_MAX = 6;
constexpr int GP_NT = 256;
constexpr int GP_PER = 4;                 // elements per thread
constexpr int GP_CHUNK = GP_NT * GP_PER;  // 1024 elements of a row per workgroup

struct GpScale {
  const float* net;   // forward: net;  backward: net
  const float* eps;
  const float* gz;    // backward only (may be NULL: zero)
  float* out;         // forward: z;  backward: gnet
  long net_bs, eps_bs, gz_bs, out_bs;
  long row;           // 2 h w
  int nk;             // chunks per row
  int first;          // chunks of the scales before this one
  int vec;            // float4 path
};
struct GpArgs {
  GpScale s[GP_MAX];
  int n, B;
};

// the sampler's standard deviation, stated once: forward and backward must agree bit for bit
__device__ __forceinline__ float gp_std(float logvar) { return expf(logvar / 2.0f); }

__device__ __forceinline__ bool gp_locate(const GpArgs& a, int& i, int& b, int& d, long& e0) {
  const int wg = blockIdx.x;
  i = 0;
#pragma unroll
  for (int k = 1; k < GP_MAX; ++k)
    if (k < a.n && wg >= a.s[k].first) i = k;
  const int local = wg - a.s[i].first, nk = a.s[i].nk;
  const int bd = local / nk;
  if (bd >= 2 * a.B) return false;
  b = bd >> 1, d = bd & 1;
  e0 = (long)(local % nk) * GP_CHUNK;
  return true;
}

template <bool VEC>
__device__ __forceinline__ double gp_sample_body(const GpScale& s, int b, int d, long e0) {
  const float* mean = s.net + b * s.net_bs + 2L * d * s.row;
  const float* lv = mean + s.row;
  const float* ep = s.eps + b * s.eps_bs + (long)d * s.row;
  float* z = s.out + b * s.out_bs + (long)d * s.row;
  double acc = 0.;
  if constexpr (VEC) {
    const long e = e0 + 4 * threadIdx.x;
    if (e < s.row) {  // row % 4 == 0: a group of four is inside or outside as a whole
      const float4 m = *reinterpret_cast<const float4*>(mean + e), l = *reinterpret_cast<const float4*>(lv + e),
                   n = *reinterpret_cast<const float4*>(ep + e);
      float4 r;
      const float t0 = gp_std(l.x) * n.x, t1 = gp_std(l.y) * n.y, t2 = gp_std(l.z) * n.z, t3 = gp_std(l.w) * n.w;
      r.x = m.x + t0, r.y = m.y + t1, r.z = m.z + t2, r.w = m.w + t3;
      *reinterpret_cast<float4*>(z + e) = r;
      acc = (((double)l.x + (double)l.y) + (double)l.z) + (double)l.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < GP_PER; ++j) {
      const long e = e0 + threadIdx.x + j * GP_NT;
      if (e < s.row) {
        const float l = lv[e];
        const float t = gp_std(l) * ep[e];
        z[e] = mean[e] + t;
        acc += (double)l;
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(GP_NT) void gauss_pyr_sample_kernel(const GpArgs a, double* __restrict__ work) {
  __shared__ double part[GP_NT / AF_WAVE];
  int i, b, d;
  long e0;
  if (!gp_locate(a, i, b, d, e0)) return;  // (never: the grid is the sum of the chunk counts)
  const GpScale& s = a.s[i];
  double acc[1] = {s.vec ? gp_sample_body<true>(s, b, d, e0) : gp_sample_body<false>(s, b, d, e0)};
  af_block_sum_f64<1, GP_NT>(acc, part);
  if (threadIdx.x == 0) work[blockIdx.x] = acc[0];
}

// grid (2 n), one wave: ent[i,d] = the partials of (i, b, d, k) over b then k
struct GpFold {
  int first[GP_MAX], nk[GP_MAX];
  int B;
};
__global__ __launch_bounds__(AF_WAVE) void gauss_pyr_fold_kernel(const GpFold f, const double* __restrict__ work,
                                                                 double* __restrict__ ent) {
  const int i = blockIdx.x >> 1, d = blockIdx.x & 1;
  const int nk = f.nk[i], cnt = f.B * nk;
  const double* w = work + f.first[i];
  double acc = 0.;
  for (int j = threadIdx.x; j < cnt; j += AF_WAVE) acc += w[(long)((j / nk) * 2 + d) * nk + j % nk];
  acc = af_wave_sum(acc);
  if (threadIdx.x == 0) ent[blockIdx.x] = acc;
}

template <bool VEC>
__device__ __forceinline__ void gp_bwd_body(const GpScale& s, int b, int d, long e0, float ge) {
  const float* lv = s.net + b * s.net_bs + (2L * d + 1) * s.row;
  const float* ep = s.eps + b * s.eps_bs + (long)d * s.row;
  const float* gz = s.gz ? s.gz + b * s.gz_bs + (long)d * s.row : nullptr;
  float* gmean = s.out + b * s.out_bs + 2L * d * s.row;
  float* glv = gmean + s.row;
  if constexpr (VEC) {
    const long e = e0 + 4 * threadIdx.x;
    if (e >= s.row) return;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gz) g = *reinterpret_cast<const float4*>(gz + e);
    const float4 l = *reinterpret_cast<const float4*>(lv + e), n = *reinterpret_cast<const float4*>(ep + e);
    float4 r;
    const float t0 = g.x * (0.5f * gp_std(l.x) * n.x), t1 = g.y * (0.5f * gp_std(l.y) * n.y),
                t2 = g.z * (0.5f * gp_std(l.z) * n.z), t3 = g.w * (0.5f * gp_std(l.w) * n.w);
    r.x = t0 + ge, r.y = t1 + ge, r.z = t2 + ge, r.w = t3 + ge;
    *reinterpret_cast<float4*>(gmean + e) = g;
    *reinterpret_cast<float4*>(glv + e) = r;
  } else {
#pragma unroll
    for (int j = 0; j < GP_PER; ++j) {
      const long e = e0 + threadIdx.x + j * GP_NT;
      if (e < s.row) {
        const float g = gz ? gz[e] : 0.f;
        const float t = g * (0.5f * gp_std(lv[e]) * ep[e]);
        gmean[e] = g;
        glv[e] = t + ge;
      }
    }
  }
}

__global__ __launch_bounds__(GP_NT) void gauss_pyr_bwd_kernel(const GpArgs a, const double* __restrict__ gent) {
  int i, b, d;
  long e0;
  if (!gp_locate(a, i, b, d, e0)) return;
  const GpScale& s = a.s[i];
  const float ge = gent ? (float)gent[2 * i + d] : 0.f;
  if (s.vec)
    gp_bwd_body<true>(s, b, d, e0, ge);
  else
    gp_bwd_body<false>(s, b, d, e0, ge);
}

// sizes -> rows, chunk counts and the prefix table; the total chunk count in *total
inline int gp_layout(const int* h, const int* w, int n, int B, GpArgs& a, long* total) {
  AF_REQUIRE_PTR(h);
  AF_REQUIRE_PTR(w);
  AF_REQUIRE(n >= 1 && n <= GP_MAX, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && B <= 65535, ARFLOW_ESHAPE);
  long sum = 0;
  for (int i = 0; i < n; ++i) {
    AF_REQUIRE(h[i] >= 1 && w[i] >= 1 && (long)h[i] * w[i] <= 0x3fffffffL, ARFLOW_ESHAPE);
    a.s[i].row = 2L * h[i] * w[i];
    a.s[i].nk = af_cdiv(a.s[i].row, GP_CHUNK);
    a.s[i].first = (int)sum;
    sum += 2L * B * a.s[i].nk;
    AF_REQUIRE(sum <= 0x7fffffffL, ARFLOW_ESHAPE);
  }
  a.n = n, a.B = B;
  *total = sum;
  return ARFLOW_OK;
}

}  // namespace

extern "C" long arflow_gauss_pyr_work_size(const int* h, const int* w, int n, int B) {
  GpArgs a;
  long total = 0;
  const int rc = gp_layout(h, w, n, B, a, &total);
  return rc != ARFLOW_OK ? rc : total;
}

extern "C" int arflow_gauss_pyr_sample_fwd(const float* const* net, const long* net_bs, const float* const* eps,
                                           const long* eps_bs, float* const* z, const long* z_bs, const int* h, const int* w,
                                           int n, int B, double* work, double* ent, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(net);
  AF_REQUIRE_PTR(net_bs);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(eps_bs);
  AF_REQUIRE_PTR(z);
  AF_REQUIRE_PTR(z_bs);
  AF_REQUIRE_PTR(work);
  AF_REQUIRE_PTR(ent);
  GpArgs a = {};
  long total = 0;
  const int rc = gp_layout(h, w, n, B, a, &total);
  if (rc != ARFLOW_OK) return rc;
  GpFold f = {};
  f.B = B;
  for (int i = 0; i < n; ++i) {
    AF_REQUIRE_PTR(net[i]);
    AF_REQUIRE_PTR(eps[i]);
    AF_REQUIRE_PTR(z[i]);
    GpScale& s = a.s[i];
    AF_REQUIRE(af_stride_ok(net_bs[i], B, 4 * s.row) && af_stride_ok(eps_bs[i], B, 2 * s.row) &&
                   af_stride_ok(z_bs[i], B, 2 * s.row), ARFLOW_ESHAPE);
    s.net = net[i], s.eps = eps[i], s.gz = nullptr, s.out = z[i];
    s.net_bs = net_bs[i], s.eps_bs = eps_bs[i], s.gz_bs = 0, s.out_bs = z_bs[i];
    s.vec = (s.row / 2) % 4 == 0 && af_vec4_ok(net[i], net_bs[i], B) && af_vec4_ok(eps[i], eps_bs[i], B) &&
            af_vec4_ok(z[i], z_bs[i], B);
    f.first[i] = s.first, f.nk[i] = s.nk;
  }
  hipLaunchKernelGGL(gauss_pyr_sample_kernel, dim3((unsigned)total), dim3(GP_NT), 0, (hipStream_t)stream, a, work);
  AF_LAUNCH_CHECK();
  hipLaunchKernelGGL(gauss_pyr_fold_kernel, dim3(2 * n), dim3(AF_WAVE), 0, (hipStream_t)stream, f, work, ent);
  return af_launch_status();
}

extern "C" int arflow_gauss_pyr_sample_bwd(const float* const* gz, const long* gz_bs, const float* const* net,
                                           const long* net_bs, const float* const* eps, const long* eps_bs, const double* gent,
                                           float* const* gnet, const long* gnet_bs, const int* h, const int* w, int n, int B,
                                           arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(net);
  AF_REQUIRE_PTR(net_bs);
  AF_REQUIRE_PTR(eps);
  AF_REQUIRE_PTR(eps_bs);
  AF_REQUIRE_PTR(gnet);
  AF_REQUIRE_PTR(gnet_bs);
  if (gz) AF_REQUIRE_PTR(gz_bs);
  GpArgs a = {};
  long total = 0;
  const int rc = gp_layout(h, w, n, B, a, &total);
  if (rc != ARFLOW_OK) return rc;
  for (int i = 0; i < n; ++i) {
    AF_REQUIRE_PTR(net[i]);
    AF_REQUIRE_PTR(eps[i]);
    AF_REQUIRE_PTR(gnet[i]);
    GpScale& s = a.s[i];
    const float* g = gz ? gz[i] : nullptr;
    AF_REQUIRE(af_stride_ok(net_bs[i], B, 4 * s.row) && af_stride_ok(eps_bs[i], B, 2 * s.row) &&
                   af_stride_ok(gnet_bs[i], B, 4 * s.row) && (!g || af_stride_ok(gz_bs[i], B, 2 * s.row)), ARFLOW_ESHAPE);
    s.net = net[i], s.eps = eps[i], s.gz = g, s.out = gnet[i];
    s.net_bs = net_bs[i], s.eps_bs = eps_bs[i], s.gz_bs = g ? gz_bs[i] : 0, s.out_bs = gnet_bs[i];
    s.vec = (s.row / 2) % 4 == 0 && af_vec4_ok(net[i], net_bs[i], B) && af_vec4_ok(eps[i], eps_bs[i], B) &&
            af_vec4_ok(gnet[i], gnet_bs[i], B) && (!g || af_vec4_ok(g, gz_bs[i], B));
  }
  hipLaunchKernelGGL(gauss_pyr_bwd_kernel, dim3((unsigned)total), dim3(GP_NT), 0, (hipStream_t)stream, a, gent);
  return af_launch_status();
}
