// Permutation passes between the phase-mosaic layouts of the dilated context layers (phase_plan.hpp),
// for gfx950.  The split-bf16 convolution kernels stay dilation-1: a layer with dilation d runs on its input REARRANGED so that
// every phase x[:, :, p::d, q::d] is a cell of a virtual image; these two kernels rearrange -- from the layout of one layer to
// the layout of the next -- where the composed path has its bias / LeakyReLU passes:
//   phase_move      dst = src, read in layout d_src and written in layout d_dst (and, optionally, in a second layout as well);
//   phase_act_bwd   gin = gout * (y > 0 ? 1 : slope), gout and y in one layout, gin in another, plus the bias gradient.
// Every separator and ragged-tail element of a destination is WRITTEN AS ZERO (it is the next convolution's padding); those
// of a source are never loaded: they hold whatever a convolution stored there.
//
// One pass: a workgroup owns RB real rows (n, c, h0 .. h0 + RB), a wave RW of them.  A real row is, in any layout, d / Qg
// contiguous virtual rows (one per group of column phases), so both sides move whole rows.  Where the elements of such a row
// sit does not depend on the row: the workgroup first writes the column map of each layout -- offset from the row's first
// segment and real column, or -1 for a separator or a tail -- into LDS (the two integer divisions per element are paid once
// per workgroup, not once per row), then every wave loads its rows' source segments, the RW loads of a trip going out
// together, drops every real element at its real column in LDS, and writes the destination segments from there, zeros
// where the map says separator or tail.  Rows h >= H are no real rows: they name the separator and tail rows of a
// destination, which are written as zeros without a load.
//
// The bias gradient is summed over the elements that were loaded, i.e. by POSITION over real pixels, in float64 from the first
// addition as arflow_bias_act_bwd's fixed-order kernel does (bias_grad_det_kernel, act.hip): per thread, then af_block_sum_f64,
// one partial per workgroup and channel stored to `rows` ([N * gridDim.x][C] doubles, every row written); the caller adds the
// rows in a fixed order.  No atomics: the same bits in either mode.
#include <climits>

#include "common.hpp"
#include "phase_plan.hpp"

namespace {
using phase_plan::Plan;

constexpr int NT = 256, NW = NT / 64;
constexpr int RW = 8;                      // rows per wave: the loads in flight per lane
constexpr int RB = RW * NW;                // rows per workgroup
constexpr int MAX_LDS = 160 * 1024 - 128;  // dynamic LDS a workgroup may ask for (the reduction's scratch is static)

struct Ent {  // one element of a real row in a layout
  int off;    // from the row's first segment, in floats
  int w;      // where the staged row keeps it (lds_column of the real column), -1: separator or ragged tail
};
struct Seg {  // the virtual rows of one real row start at base (+ Ent::off)
  long base;
  bool exists;
};
__device__ __forceinline__ Seg segments(const Plan& p, int C, int n, int c, int h) {
  const phase_plan::Row r = phase_plan::row_to_virtual(p, h);
  const long plane = (long)p.Hv * p.Wv;
  Seg s;
  s.exists = r.hv < p.Hv;  // false for the row below the last cell: no separator follows it
  s.base = ((long)phase_plan::sample_to_virtual(p, n, r.g, 0) * C + c) * plane + (long)r.hv * p.Wv;
  return s;
}
PHASE_HD inline int row_elements(const Plan& p) { return (p.d / p.Qg) * p.Wv; }
// the rows a layout names: the real ones, its tail rows and -- where cells are stacked -- the separator rows below them
PHASE_HD inline int named_rows(const Plan& p) { return (p.Pg == 1 ? p.Hs : p.Hs + 1) * p.d; }

// A staged row keeps real column w at float w + w / 32: lanes that walk a cell touch columns d apart, and one spare float per
// 32 puts the strides 2 .. 16 of the layouts on different banks (stride 16: banks 0, 16, 1, 17, ... instead of two).
PHASE_HD inline int lds_column(int w) { return w + (w >> 5); }
PHASE_HD inline int lds_pitch(int W) { return lds_column(W - 1) + 1; }

__device__ __forceinline__ void column_map(const Plan& p, int C, Ent* __restrict__ tab) {
  const int n = row_elements(p), step = C * p.Hv * p.Wv;  // a whole layout holds at most INT_MAX floats (host-checked)
  for (int t = threadIdx.x; t < n; t += NT) {
    const int g = t / p.Wv, wv = t - g * p.Wv;
    const int w = phase_plan::col_to_real(p, g, wv);
    tab[t] = {g * step + wv, w < 0 ? -1 : lds_column(w)};
  }
}

template <bool ACT>
__global__ __launch_bounds__(NT) void phase_kernel(const float* __restrict__ src, const float* __restrict__ act, float* __restrict__ dst,
                                                   float* __restrict__ dst2, double* __restrict__ rows, Plan ps, Plan pd, Plan pd2,
                                                   int C, float slope) {
  extern __shared__ __align__(8) float lds[];
  __shared__ double red[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y, n = blockIdx.z;
  const int h0 = blockIdx.x * RB + wave * RW;
  const int H = ps.H, W = lds_pitch(ps.W);
  float* const mine = lds + (size_t)wave * RW * W;
  const int nsrc = row_elements(ps), nd = row_elements(pd);
  Ent* const tsrc = reinterpret_cast<Ent*>(lds + (size_t)RB * W);
  Ent* const tdst = tsrc + nsrc;
  Ent* const tdst2 = tdst + nd;
  column_map(ps, C, tsrc);
  column_map(pd, C, tdst);
  if (dst2) column_map(pd2, C, tdst2);
  __syncthreads();

  double s[1] = {0.0};
  if (h0 < H) {
    long base[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) base[r] = segments(ps, C, n, c, min(h0 + r, H - 1)).base;  // clamped: every address lies inside src
    for (int t = lane; t < nsrc; t += 64) {
      const Ent e = tsrc[t];
      if (e.w < 0) continue;
      float v[RW], a[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        v[r] = src[base[r] + e.off];
        a[r] = ACT ? act[base[r] + e.off] : 1.f;
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        if (ACT) {
          v[r] = a[r] > 0.f ? v[r] : v[r] * slope;
          if (h0 + r < H) s[0] += (double)v[r];
        }
        mine[r * W + e.w] = v[r];
      }
    }
  }
  __syncthreads();

  const auto put = [&](float* __restrict__ out, const Plan& p, const Ent* __restrict__ tab, int ne) {
    const int hend = named_rows(p);
    if (h0 >= hend) return;
    Seg o[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) o[r] = segments(p, C, n, c, min(h0 + r, hend - 1));
    for (int t = lane; t < ne; t += 64) {
      const Ent e = tab[t];
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        if (h0 + r >= hend || !o[r].exists) continue;
        out[o[r].base + e.off] = e.w >= 0 && h0 + r < H ? mine[r * W + e.w] : 0.f;
      }
    }
  };
  put(dst, pd, tdst, nd);
  if (dst2) put(dst2, pd2, tdst2, row_elements(pd2));

  if (ACT && rows) {
    af_block_sum_f64<1, NT>(s, red);
    if (threadIdx.x == 0) rows[((long)n * gridDim.x + blockIdx.x) * C + c] = s[0];
  }
}

// the rows a launch walks: the real rows and, below them, the names of every destination's separator and tail rows
inline int walked_rows(const Plan& pd, const Plan* pd2) {
  int h = named_rows(pd);
  if (pd2 && named_rows(*pd2) > h) h = named_rows(*pd2);
  return h;
}
inline bool layout_ok(int N, int C, int H, int W, int d) {
  if (!(C > 0 && C <= 65535 && N <= 65535 && phase_plan::shape_ok(N, H, W, d))) return false;
  return phase_plan::elements(phase_plan::make_plan(N, H, W, d), C) <= INT_MAX;
}

template <bool ACT>
int launch(const float* src, const float* act, float* dst, float* dst2, double* rows, int N, int C, int H, int W, int d_src, int d_dst,
           int d_dst2, float slope, hipStream_t st) {
  AF_REQUIRE(layout_ok(N, C, H, W, d_src) && layout_ok(N, C, H, W, d_dst) && (!dst2 || layout_ok(N, C, H, W, d_dst2)), ARFLOW_ESHAPE);
  const Plan ps = phase_plan::make_plan(N, H, W, d_src), pd = phase_plan::make_plan(N, H, W, d_dst);
  const Plan pd2 = dst2 ? phase_plan::make_plan(N, H, W, d_dst2) : pd;
  const long bytes = sizeof(float) * (long)RB * lds_pitch(W) + sizeof(Ent) * ((long)row_elements(ps) + row_elements(pd) + (dst2 ? row_elements(pd2) : 0));
  AF_REQUIRE(bytes <= MAX_LDS, ARFLOW_ESHAPE);
  if (bytes > 64 * 1024) {  // long rows only (W beyond about 350): asked for on the current device at every such launch, no state kept
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&phase_kernel<ACT>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS);
    if (e != hipSuccess) return af_hip_status(e);
  }
  const dim3 grid((unsigned)af_cdiv(walked_rows(pd, dst2 ? &pd2 : nullptr), RB), (unsigned)C, (unsigned)N);
  hipLaunchKernelGGL(phase_kernel<ACT>, grid, dim3(NT), (size_t)bytes, st, src, act, dst, dst2, rows, ps, pd, pd2, C, slope);
  return af_launch_status();
}
}  // namespace

extern "C" int arflow_phase_layout(int N, int H, int W, int d, int* nv_hv_wv_pg_qg) {
  AF_REQUIRE_PTR(nv_hv_wv_pg_qg);
  AF_REQUIRE(phase_plan::shape_ok(N, H, W, d), ARFLOW_ESHAPE);
  const Plan p = phase_plan::make_plan(N, H, W, d);
  nv_hv_wv_pg_qg[0] = p.Nv, nv_hv_wv_pg_qg[1] = p.Hv, nv_hv_wv_pg_qg[2] = p.Wv, nv_hv_wv_pg_qg[3] = p.Pg, nv_hv_wv_pg_qg[4] = p.Qg;
  return ARFLOW_OK;
}

extern "C" int arflow_phase_rows(int N, int H, int W, int d_dst, int d_dst2) {
  AF_REQUIRE(phase_plan::shape_ok(N, H, W, d_dst) && (d_dst2 == 0 || phase_plan::shape_ok(N, H, W, d_dst2)), ARFLOW_ESHAPE);
  const Plan pd = phase_plan::make_plan(N, H, W, d_dst), pd2 = phase_plan::make_plan(N, H, W, d_dst2 ? d_dst2 : d_dst);
  return N * af_cdiv(walked_rows(pd, &pd2), RB);
}

extern "C" int arflow_phase_move(const float* src, float* dst, float* dst2, int N, int C, int H, int W, int d_src, int d_dst,
                                 int d_dst2, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(src);
  AF_REQUIRE_PTR(dst);
  AF_REQUIRE((dst2 == nullptr) == (d_dst2 == 0), ARFLOW_EPARAM);
  return launch<false>(src, nullptr, dst, dst2, nullptr, N, C, H, W, d_src, d_dst, d_dst2, 0.f, (hipStream_t)stream);
}

extern "C" int arflow_phase_act_bwd(const float* gout, const float* y, float* gin, float* gin2, double* rows, int N, int C, int H,
                                    int W, int d_a, int d_b, int d_b2, float negative_slope, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(gout);
  AF_REQUIRE_PTR(y);
  AF_REQUIRE_PTR(gin);
  AF_REQUIRE((gin2 == nullptr) == (d_b2 == 0), ARFLOW_EPARAM);
  return launch<true>(gout, y, gin, gin2, rows, N, C, H, W, d_a, d_b, d_b2, negative_slope, (hipStream_t)stream);
}
