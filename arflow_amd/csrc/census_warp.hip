// Fused photometric direction of UFlowLoss (losses/uflow_loss.py:30-54) for gfx950:
//
//     recons = resample(im_b, flow_to_warp(flow))                     utils/uflow_utils.py:6-32,53-77
//     valid  = mask_invalid(flow_to_warp(flow))                       utils/uflow_utils.py:35-50
//     mask   = upsample(clamp(range_map, 0, 1), x4) * valid           losses/uflow_loss.py:41-48
//     loss   = census_loss(im_a, recons, mask)                        utils/uflow_utils.py:282-293
//
// as ONE forward launch and ONE backward launch.  Unfused this was warp_fwd (24-30 us at 8x3x384x640) ->
// up4_clamp_mul -> census_fwd forward and census_bwd -> warp_bwd_flow (25-27 us) backward, with the warped image,
// the validity mask and the image gradient making a round trip through HBM in between.
//
// The census transform only sees the GREY image (rgb_to_grayscale, utils/uflow_utils.py:227-231) and both the
// bilinear sample and the grey conversion are linear, so grey(resample(im_b)) = resample(grey(im_b)): the kernels
// take the grey planes (x255) of the two images -- written once per step by arflow_down4_gray, which reads the
// images anyway for the x1/4 copies of the smoothness term -- and sample ONE plane (4 taps) while the tile is
// filled instead of three.  The warped image, its gradient and the validity mask never exist in memory; the
// backward turns the per-pixel grey gradient straight into d loss / d flow with the bilinear corner differences
// of the grey plane.  (The re-association changes results at fp32 rounding level only; the unfused entry points
// keep the reference's operation order and tests/test_hip_parity.py compares the two and the oracle.)
//
// The census arithmetic (census4 of photo.hip: 16 x 64 pixel tile, 4 pixels per lane, window rows as
// ds_read_b128) is transcendental/VALU-bound; the ~6 extra dword gathers per pixel of the fill stage (tile + 3 px
// halo = 1.5 x the tile, 4 taps each) are served by L2 and overlap other workgroups' arithmetic.
#include <cstdlib>

#include "census_tile.hpp"
#include "smooth_dev.hpp"
#include "taps.hpp"

namespace {
namespace census_warp {
using namespace census4;

// Grey tile of the WARPED image b: rows [ty0-R, ty0+TYH+R), columns [tx0-R, tx0+TXW+R); zero outside the image
// (the census transform zero-pads).  All flow loads of a thread are issued together, then all its 4 x ITER taps:
// two round trips for the whole fill instead of a dependent chain per pixel.
template <int R>
__device__ __forceinline__ void load_gray_warped(float* __restrict__ tile, const float* __restrict__ gsrc,
                                                 const float* __restrict__ flow, int H, int W, int ty0, int tx0) {
  constexpr int NR = TYH + 2 * R, NC = TXW + 2 * R, ITER = (NR * NC + NT - 1) / NT;
  const long cs = (long)H * W;
  float u[ITER], v[ITER];
  int gx[ITER], gy[ITER];
  bool in[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k) {
    const int i = threadIdx.x + k * NT;
    const int r = i / NC, c = i - r * NC;
    gy[k] = ty0 - R + r;
    gx[k] = tx0 - R + c;
    in[k] = i < NR * NC && gy[k] >= 0 && gy[k] < H && gx[k] >= 0 && gx[k] < W;
    const long o = in[k] ? (long)gy[k] * W + gx[k] : 0;
    u[k] = flow[o];
    v[k] = flow[o + cs];
  }
  float a[ITER][4];
  TapPlan p[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k) {
    const Taps t = make_taps((float)gx[k], (float)gy[k], u[k], v[k], H, W, H, W, ARFLOW_PAD_ZEROS, true, ARFLOW_NORM_UFLOW);
    p[k] = plan_taps(t, H, W);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[k][q] = gsrc[p[k].o[q]];
  }
#pragma unroll
  for (int k = 0; k < ITER; ++k) {
    const int i = threadIdx.x + k * NT;
    const int r = i / NC, c = i - r * NC;
    if (i < NR * NC) tile[r * PITCH + (c + 4 - R)] = in[k] ? tap_blend(p[k], a[k]) : 0.f;
  }
}

// zero the tile columns no gather fills (tile col 0 .. 3-R and 4+TXW+R .. TXW+7): read12 loads them
template <int R>
__device__ __forceinline__ void zero_margins(float* __restrict__ tile) {
  constexpr int NR = TYH + 2 * R, M = 4 - R;
  for (int i = threadIdx.x; i < NR * 2 * M; i += NT) {
    const int r = i / (2 * M), c = i - r * (2 * M);
    tile[r * PITCH + (c < M ? c : TXW + 4 + R + (c - M))] = 0.f;
  }
}

template <int R>
__global__ __launch_bounds__(NT) void fwd_kernel(const float* __restrict__ gray_a, const float* __restrict__ gray_b,
                                                 const float* __restrict__ flow, long fbs,
                                                 const float* __restrict__ occ_small, float* __restrict__ mask_out,
                                                 float* __restrict__ dham_out, float* __restrict__ sums, int nrows,
                                                 int nimg, int H, int W, int pair) {
  // pair: the batch interleaves the two DIRECTIONS of UFlowLoss (sample s = 2 b + dir; losses/uflow_loss.py:30-54 runs them
  // one after the other): image b of sample s is plane s ^ 1 of `gray_b` (= gray_a), its range map plane s ^ 1 of
  // `occ_small`, and the partial sums of direction 1 go to columns 2, 3 of the row instead of 0, 1.
  __shared__ __attribute__((aligned(16))) float ga[ROWS * PITCH];
  __shared__ __attribute__((aligned(16))) float gb[ROWS * PITCH];
  __shared__ float red[2 * (NT / 64)];
  int btx, bty, b;
  if (!af_tile_of_block((W + TXW - 1) / TXW, (H + TYH - 1) / TYH, nimg, btx, bty, b)) {
    if (threadIdx.x == 0) af_store_partial(sums, nrows, 0.f, 0.f, 0.f);  // padding workgroup: its row must be defined
    return;
  }
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)H * W;
  const float* fl = flow + b * fbs;
  const int bp = pair ? (b ^ 1) : b;
  zero_margins<R>(gb);
  load_gray_warped<R>(gb, gray_b + bp * cs, fl, H, W, ty0, tx0);
  load_plane<R>(ga, gray_a + b * cs, H, W, ty0, tx0);
  __syncthreads();
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  float ca[4], cb[4], s[4] = {0.f, 0.f, 0.f, 0.f};
  {
    float wa[12], wb[12];
    read12(ga + (ly + R) * PITCH + 4 * xg, wa);
    read12(gb + (ly + R) * PITCH + 4 * xg, wb);
#pragma unroll
    for (int p = 0; p < 4; ++p) ca[p] = wa[4 + p], cb[p] = wb[4 + p];
  }
#pragma unroll 1
  for (int dy = 0; dy <= 2 * R; ++dy) {
    float wa[12], wb[12];
    read12(ga + (ly + dy) * PITCH + 4 * xg, wa);
    read12(gb + (ly + dy) * PITCH + 4 * xg, wb);
#pragma unroll
    for (int dx = 0; dx <= 2 * R; ++dx)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int k = p + dx + 4 - R;
        s[p] = pair_dist_acc(ca[p], cb[p], wa[k], wb[k], s[p]);
      }
  }
  float part[2] = {0.f, 0.f};
  if (y < H && x0 < W) {  // W % 4 == 0: the 4 pixels are inside together
    const long o = (long)y * W + x0;
    const float* occ = occ_small ? occ_small + (long)bp * (H / 4) * (W / 4) : nullptr;
    float mv[4], dh[4];
    masked_loss4(fl, occ, s, x0, y, H, W, R, mv, dh, part);
    if (mask_out) store_row<4>(mask_out + (long)b * cs + o, mv);
    store_row<4>(dham_out + (long)b * cs + o, dh);
  }
  af_block_sum<2>(part, red);
  if (threadIdx.x == 0) store_dir_partial(sums, nrows, part, pair, b);
}

template <int R>
__device__ __forceinline__ void bwd_body(const float* __restrict__ gray_a, const float* __restrict__ gray_b,
                                         const float* __restrict__ flow, long fbs,
                                         const float* __restrict__ dham, const float* __restrict__ scale,
                                         float* __restrict__ gflow, int nimg, int H, int W, int pair) {
  __shared__ __attribute__((aligned(16))) float ga[ROWS * PITCH];
  __shared__ __attribute__((aligned(16))) float gb[ROWS * PITCH];
  __shared__ __attribute__((aligned(16))) float gg[ROWS * PITCH];
  int btx, bty, b;
  if (!af_tile_of_block((W + TXW - 1) / TXW, (H + TYH - 1) / TYH, nimg, btx, bty, b)) return;
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)H * W;
  const float* fl = flow + b * fbs;
  const float* sb = gray_b + (pair ? (b ^ 1) : b) * cs;
  zero_margins<R>(gb);
  load_gray_warped<R>(gb, sb, fl, H, W, ty0, tx0);
  load_plane<R>(ga, gray_a + b * cs, H, W, ty0, tx0);
  load_plane<R>(gg, dham + b * cs, H, W, ty0, tx0);
  __syncthreads();
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  if (y >= H || x0 >= W) return;
  // the taps of this lane's 4 pixels (corner differences of the grey plane): issued before the census loop so
  // the 16 gathers are in flight while it runs
  float cdx[4], cdy[4];
  corner_grads4(sb, fl, x0, y, H, W, cdx, cdy);
  float ca[4], cb[4], cg[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
  {
    float wa[12], wb[12], wg[12];
    read12(ga + (ly + R) * PITCH + 4 * xg, wa);
    read12(gb + (ly + R) * PITCH + 4 * xg, wb);
    read12(gg + (ly + R) * PITCH + 4 * xg, wg);
#pragma unroll
    for (int p = 0; p < 4; ++p) ca[p] = wa[4 + p], cb[p] = wb[4 + p], cg[p] = wg[4 + p];
  }
#pragma unroll 1
  for (int dy = 0; dy <= 2 * R; ++dy) {
    float wa[12], wb[12], wg[12];
    read12(ga + (ly + dy) * PITCH + 4 * xg, wa);
    read12(gb + (ly + dy) * PITCH + 4 * xg, wb);
    read12(gg + (ly + dy) * PITCH + 4 * xg, wg);
#pragma unroll
    for (int dx = 0; dx <= 2 * R; ++dx) {
      if (dy == R && dx == R) continue;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int k = p + dx + 4 - R;
        acc[p] = fmaf(wg[k] + cg[p], pair_grad(ca[p], cb[p], wa[k], wb[k]), acc[p]);
      }
    }
  }
  // d loss / d grey_b(p) = sc * acc (census4::bwd_kernel's value before the colour weights; the x255 lives in the
  // grey plane), times the warp's flow gradient
  store_flow_grad<4>(gflow + (long)b * 2 * cs + (long)y * W + x0, cs, dir_scale(scale, pair, b), acc, cdx, cdy);
}

template <int R>
__global__ __launch_bounds__(NT) void bwd_kernel(const float* __restrict__ gray_a, const float* __restrict__ gray_b,
                                                 const float* __restrict__ flow, long fbs,
                                                 const float* __restrict__ dham, const float* __restrict__ scale,
                                                 float* __restrict__ gflow, int nimg, int H, int W, int pair) {
  bwd_body<R>(gray_a, gray_b, flow, fbs, dham, scale, gflow, nimg, H, W, pair);
}

// The WHOLE backward of UFlowLoss as one launch: workgroups [0, census_blocks) run the census + warp backward of both
// directions (bwd_body, pair form), the rest the smoothness backward of the level-2 flows (smooth_bwd_pixel: one row of
// 256 columns per workgroup) -- two independent kernels that used to pay two launch latencies back to back.
template <int R>
__global__ __launch_bounds__(NT) void pair_bwd_smooth_kernel(const float* __restrict__ gray, const float* __restrict__ flow,
                                                             long fbs, const float* __restrict__ dham,
                                                             const float* __restrict__ scale2, float* __restrict__ gflow,
                                                             int nimg, int H, int W, unsigned census_blocks, SmoothArgs sa,
                                                             const float* __restrict__ coef, float* __restrict__ gflow2) {
  if (blockIdx.x < census_blocks) {
    bwd_body<R>(gray, gray, flow, fbs, dham, scale2, gflow, nimg, H, W, 1);
    return;
  }
  smooth_bwd_role(sa, coef, gflow2, nimg, blockIdx.x - census_blocks);
}

// grey plane (x255) of an RGB image and, optionally, its bilinear x1/4 copy (align_corners=False on a multiple-of-4
// grid = the mean of the central 2 x 2 of every 4 x 4 block, as down4_kernel of smooth.hip): one thread per 4 x 4
// block, every load and store a float4.
// zero (nullable): a [B, H/4, W/4] plane cleared by the same launch (the range-map accumulation target of the splat that
// follows: saves its fill launch)
__global__ __launch_bounds__(256) void down4_gray_kernel(const float* __restrict__ im, float* __restrict__ small,
                                                        float* __restrict__ gray, int H, int W,
                                                        float* __restrict__ zero = nullptr) {
  const int h = H / 4, w = W / 4;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= w) return;
  if (zero) zero[((long)b * h + y) * w + x] = 0.f;
  const long cs = (long)H * W;
  const float* p = im + (long)b * 3 * cs + (long)(4 * y) * W + 4 * x;
  float4 px[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) px[c][r] = *reinterpret_cast<const float4*>(p + c * cs + (long)r * W);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    *reinterpret_cast<float4*>(gray + (long)b * cs + (long)(4 * y + r) * W + 4 * x) = gray255(px[0][r], px[1][r], px[2][r]);
  }
  if (small) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      small[(((long)b * 3 + c) * h + y) * w + x] =
          0.5f * (0.5f * px[c][1].y + 0.5f * px[c][1].z) + 0.5f * (0.5f * px[c][2].y + 0.5f * px[c][2].z);
  }
}

}  // namespace census_warp
}  // namespace

// Pair-symmetric kernels (census_sym.hip): every unordered pixel pair evaluated once, the value handed to the other
// end through LDS -- half the transcendentals.  Built, parity-green and MEASURED slower than the ordered-pair kernels
// of this file at the BASELINE shape (8x384x640: forward 76 us vs 58 us, backward 89 us vs 69 us), so
// they are opt-in: ARFLOW_CENSUS_SYM=1 selects them (tests run both, tools/kbench.py times both).
int census_sym_fwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* occ_small,
                   float* mask_out, float* dham, float* sums, int nrows, int B, int H, int W, int radius, hipStream_t st);
int census_sym_bwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* dham,
                   const float* scale, float* gflow, int B, int H, int W, int radius, hipStream_t st);
static bool use_sym() {
  const char* e = getenv("ARFLOW_CENSUS_SYM");
  return e && e[0] == '1';
}
// The pair-shared column kernels (census_col.hpp) are the default; ARFLOW_CENSUS_COL=0 selects the ordered-pair kernels of
// this file (tests run both, tools/kbench.py times both).
static bool use_col(bool backward = false) {
  const char* e = getenv("ARFLOW_CENSUS_COL");  // 0: neither, f: forward only, 1 / unset: both
  if (e && e[0] == '0') return false;
  if (e && e[0] == 'f') return !backward;
  return true;
}
// census_col.hip
int census_col_fwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* occ_small,
                   float* mask_out, float* dham, float* sums, int nrows, int B, int H, int W, int radius, int pair,
                   hipStream_t st);
int census_col_bwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* dham,
                   const float* scale, float* gflow, int B, int H, int W, int radius, int pair, hipStream_t st);
int census_col_pair_bwd_smooth(const float* gray, const float* flow, long fbs, const float* dham, const float* scale2,
                               float* gflow, int B2, int H, int W, int radius, const float* flow2, long flow2_bstride,
                               const float* img2, int h2, int w2, float flow_scale, float alpha, int order, int wmode,
                               int penalty, const float* coef2, float* gflow2, hipStream_t st);

extern "C" int arflow_census_warp_supported(int H, int W) { return (W % 4 == 0 && H % 4 == 0 && H >= 8 && W >= 8) ? 1 : 0; }

extern "C" int arflow_down4_gray_z(const float* im, float* small, float* gray, float* zero_plane, int B, int H, int W,
                                   arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(im);
  AF_REQUIRE_PTR(gray);
  AF_REQUIRE(B > 0 && B <= 65535 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0 && H / 4 <= 65535, ARFLOW_ESHAPE);
  hipLaunchKernelGGL(census_warp::down4_gray_kernel, dim3(af_cdiv(W / 4, 256), H / 4, B), dim3(256), 0,
                     (hipStream_t)stream, im, small, gray, H, W, zero_plane);
  return af_launch_status();
}
extern "C" int arflow_down4_gray(const float* im, float* small, float* gray, int B, int H, int W, arflow_stream_t stream) {
  return arflow_down4_gray_z(im, small, gray, nullptr, B, H, W, stream);
}

// what the fused entry points require of their shared arguments (p4, p5: dham and sums / gflow)
static int census_warp_check(const float* gray_a, const float* gray_b, const float* flow, const float* p4, const float* p5,
                             long flow_bstride, int B, int H, int W, int radius) {
  AF_REQUIRE_PTR(gray_a);
  AF_REQUIRE_PTR(gray_b);
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(p4);
  AF_REQUIRE_PTR(p5);
  AF_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 8 * 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(arflow_census_warp_supported(H, W), ARFLOW_ESHAPE);
  AF_REQUIRE(flow_bstride >= 2L * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(radius >= 1 && radius <= 3, ARFLOW_EPARAM);
  return ARFLOW_OK;
}

static int census_warp_fwd_impl(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H,
                                int W, int radius, arflow_stream_t stream, int pair) {
  af_clear_stale_error();
  if (const int rc = census_warp_check(gray_a, gray_b, flow, dham, sums, flow_bstride, B, H, W, radius)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nrows = af_sums_rows(B, H, W);
  if (use_sym() && !pair) return census_sym_fwd(gray_a, gray_b, flow, flow_bstride, occ_small, mask_out, dham, sums, nrows, B, H, W, radius, st);
  namespace cw = census_warp;
  if (use_col())
    return census_col_fwd(gray_a, gray_b, flow, flow_bstride, occ_small, mask_out, dham, sums, nrows, B, H, W, radius, pair, st);
  af_dispatch_radius(radius, [&](auto R) {
    hipLaunchKernelGGL(cw::fwd_kernel<decltype(R)::value>, dim3(cw::grid(B, H, W)), dim3(cw::NT), 0, st, gray_a, gray_b, flow,
                       flow_bstride, occ_small, mask_out, dham, sums, nrows, B, H, W, pair);
  });
  return af_launch_status();
}

extern "C" int arflow_census_warp_fwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                      const float* occ_small, float* mask_out, float* dham, float* sums, int B, int H,
                                      int W, int radius, arflow_stream_t stream) {
  return census_warp_fwd_impl(gray_a, gray_b, flow, flow_bstride, occ_small, mask_out, dham, sums, B, H, W, radius, stream, 0);
}
// Both directions of UFlowLoss in one launch: B = 2 x image pairs, sample s = 2 b + direction (what the model's [B,4,H,W]
// (fw, bw) flow tensor IS when viewed as [2B,2,H,W], and the [B,6,H,W] image pair viewed as [2B,3,H,W]); `gray` holds the 2B
// grey planes: image a of sample s is plane s, image b plane s ^ 1; occ_small plane s ^ 1 masks sample s; sums columns
// (0,1) belong to direction 0, (2,3) to direction 1; `scale` of the backward holds one factor per direction.
extern "C" int arflow_census_warp_pair_fwd(const float* gray, const float* flow, long flow_bstride, const float* occ_small,
                                           float* mask_out, float* dham, float* sums, int B2, int H, int W, int radius,
                                           arflow_stream_t stream) {
  AF_REQUIRE(B2 % 2 == 0, ARFLOW_ESHAPE);
  return census_warp_fwd_impl(gray, gray, flow, flow_bstride, occ_small, mask_out, dham, sums, B2, H, W, radius, stream, 1);
}

static int census_warp_bwd_impl(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                const float* dham, const float* scale, float* gflow, int B, int H, int W,
                                int radius, arflow_stream_t stream, int pair) {
  af_clear_stale_error();
  if (const int rc = census_warp_check(gray_a, gray_b, flow, dham, gflow, flow_bstride, B, H, W, radius)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (use_sym() && !pair) return census_sym_bwd(gray_a, gray_b, flow, flow_bstride, dham, scale, gflow, B, H, W, radius, st);
  namespace cw = census_warp;
  if (use_col(true)) return census_col_bwd(gray_a, gray_b, flow, flow_bstride, dham, scale, gflow, B, H, W, radius, pair, st);
  af_dispatch_radius(radius, [&](auto R) {
    hipLaunchKernelGGL(cw::bwd_kernel<decltype(R)::value>, dim3(cw::grid(B, H, W)), dim3(cw::NT), 0, st, gray_a, gray_b, flow,
                       flow_bstride, dham, scale, gflow, B, H, W, pair);
  });
  return af_launch_status();
}

extern "C" int arflow_census_warp_bwd(const float* gray_a, const float* gray_b, const float* flow, long flow_bstride,
                                      const float* dham, const float* scale, float* gflow, int B, int H, int W,
                                      int radius, arflow_stream_t stream) {
  return census_warp_bwd_impl(gray_a, gray_b, flow, flow_bstride, dham, scale, gflow, B, H, W, radius, stream, 0);
}
extern "C" int arflow_census_warp_pair_bwd(const float* gray, const float* flow, long flow_bstride, const float* dham,
                                           const float* scale2, float* gflow, int B2, int H, int W, int radius,
                                           arflow_stream_t stream) {
  AF_REQUIRE(B2 % 2 == 0, ARFLOW_ESHAPE);
  AF_REQUIRE_PTR(scale2);
  return census_warp_bwd_impl(gray, gray, flow, flow_bstride, dham, scale2, gflow, B2, H, W, radius, stream, 1);
}

// Backward of BOTH loss terms of UFlowLoss in one launch: arflow_census_warp_pair_bwd + arflow_smooth_bwd (3-channel image,
// level-2 flows [B2,2,h2,w2] with batch stride flow2_bstride); coef2 = the two smoothness-sum gradients.
extern "C" int arflow_uflow_pair_bwd(const float* gray, const float* flow, long flow_bstride, const float* dham,
                                     const float* scale2, float* gflow, int B2, int H, int W, int radius, const float* flow2,
                                     long flow2_bstride, const float* img2, const float* coef2, float* gflow2, int h2, int w2,
                                     float flow_scale, float alpha, int order, int wmode, int penalty,
                                     arflow_stream_t stream) {
  af_clear_stale_error();
  // (its own pointers and shapes first: every null pointer is reported before any shape, every shape before any parameter)
  AF_REQUIRE_PTR(gray);
  AF_REQUIRE_PTR(flow);
  AF_REQUIRE_PTR(dham);
  AF_REQUIRE_PTR(scale2);
  AF_REQUIRE_PTR(gflow);
  AF_REQUIRE_PTR(flow2);
  AF_REQUIRE_PTR(img2);
  AF_REQUIRE_PTR(coef2);
  AF_REQUIRE_PTR(gflow2);
  AF_REQUIRE(B2 % 2 == 0 && h2 > 0 && w2 > 0, ARFLOW_ESHAPE);
  AF_REQUIRE(flow2_bstride >= 2L * h2 * w2, ARFLOW_ESHAPE);
  if (const int rc = census_warp_check(gray, gray, flow, dham, gflow, flow_bstride, B2, H, W, radius)) return rc;
  AF_REQUIRE((order == 1 || order == 2) && (wmode == 0 || wmode == 1) && (penalty == 0 || penalty == 1), ARFLOW_EPARAM);
  namespace cw = census_warp;
  const SmoothArgs sa{flow2, img2, 3, h2, w2, flow2_bstride, flow_scale, alpha, order, wmode, penalty};
  hipStream_t st = (hipStream_t)stream;
  if (use_col(true)) return census_col_pair_bwd_smooth(gray, flow, flow_bstride, dham, scale2, gflow, B2, H, W, radius, flow2, flow2_bstride, img2, h2, w2,
                                                         flow_scale, alpha, order, wmode, penalty, coef2, gflow2, st);
  const unsigned cb = cw::grid(B2, H, W);
  af_dispatch_radius(radius, [&](auto R) {
    hipLaunchKernelGGL(cw::pair_bwd_smooth_kernel<decltype(R)::value>, dim3(cb + smooth_role_blocks(sa, B2)), dim3(cw::NT), 0, st,
                       gray, flow, flow_bstride, dham, scale2, gflow, B2, H, W, cb, sa, coef2, gflow2);
  });
  return af_launch_status();
}
