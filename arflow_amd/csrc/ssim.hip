// SSIM (3x3, un-padded) + L1 photometric term of the ARFlow pyramid loss for gfx950 -- forward and backward
// (losses/loss_blocks.py:65-84 SSIM, losses/flow_loss.py:13-27).  Split from photo.hip (census kernels) because the two
// want different compiler settings: these kernels are built WITHOUT the SLP vectoriser (Makefile: its v_pk_* pairing
// costs more v_mov than it saves here: forward 28.4 -> 23.5 us, backward 53.3 -> 45.6 us at 8x3x384x640), the census
// kernels with it (backward 59 -> 69 us without).
//
// The kernels here are staging (global -> LDS tiles, the block sums, the stores) plus calls: every piece of SSIM
// arithmetic, and the stages the 16 x 64 tiling shares with photo_warp.hip, are in ssim_dev.hpp.
#include "common.hpp"
#include "ssim_dev.hpp"

namespace {

constexpr int TX = 32, TY = 8;  // pixel tile = 256 threads, lanes run along x

// ------------------------------------------------------------------------------------------------
// SSIM (3x3, un-padded) + L1
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TX* TY) void photo_fwd_kernel(const float* __restrict__ im,
                                                           const float* __restrict__ rec,
                                                           const float* __restrict__ mask,
                                                           float* __restrict__ ssim_map,
                                                           float* __restrict__ sums, int nrows, int nimg, int C, int H, int W) {
  __shared__ float tx[TY + 2][TX + 3];  // x = recons*mask
  __shared__ float ty[TY + 2][TX + 3];  // y = im*mask
  __shared__ float red[3 * (TX * TY / 64)];
  int btx_, bty_, b;
  if (!af_tile_of_block((W + TX - 1) / TX, (H + TY - 1) / TY, nimg, btx_, bty_, b)) {
    if (threadIdx.x == 0) af_store_partial(sums, nrows, 0.f, 0.f, 0.f);  // padding workgroup: its row must be defined
    return;
  }
  const int ty0 = bty_ * TY, tx0 = btx_ * TX;
  const long cs = (long)H * W;
  const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
  const int x = tx0 + lx, y = ty0 + ly;
  float part[3] = {0.f, 0.f, 0.f};
  if (x < W && y < H) part[2] = mask ? mask[(long)b * cs + (long)y * W + x] : 1.f;
  for (int c = 0; c < C; ++c) {
    const float* imc = im + ((long)b * C + c) * cs;
    const float* rc = rec + ((long)b * C + c) * cs;
    __syncthreads();
    for (int idx = threadIdx.x; idx < (TY + 2) * (TX + 2); idx += TX * TY) {
      const int r = idx / (TX + 2), cc = idx - r * (TX + 2);
      const int gy = ty0 + r, gx = tx0 + cc;
      float a = 0.f, bb = 0.f;
      if (gy < H && gx < W) {
        const long o = (long)gy * W + gx;
        const float m = mask ? mask[(long)b * cs + o] : 1.f;
        const float iv = imc[o], rv = rc[o];
        a = rv * m;
        bb = iv * m;
        if (r < TY && cc < TX) part[0] += fabsf(iv - rv) * m;  // each pixel owned by exactly one tile slot
      }
      tx[r][cc] = a;
      ty[r][cc] = bb;
    }
    __syncthreads();
    if (x < W - 2 && y < H - 2) {
      const float dist = ssim_dist(window_stats<TX + 3>(tx, ty, ly, lx));
      part[1] += dist;
      if (ssim_map) ssim_map[(((long)b * C + c) * (H - 2) + y) * (W - 2) + x] = dist;
    }
  }
  af_block_sum<3>(part, red);
  if (threadIdx.x == 0) af_store_partial(sums, nrows, part[0], part[1], part[2]);
}

// d dist_w / d x_r = -(1/2) (alpha_w + beta_w x_r + gamma_w y_r) where 0 <= (1-S)/2 <= 1, else 0.
__global__ __launch_bounds__(TX* TY) void photo_bwd_kernel(const float* __restrict__ im,
                                                           const float* __restrict__ rec,
                                                           const float* __restrict__ mask,
                                                           const float* __restrict__ gmap,
                                                           const float* __restrict__ coef,
                                                           float* __restrict__ g_rec, int nimg, int C, int H, int W) {
  // data region: pixels (ty0-2 .. ty0+TY+1) x (tx0-2 .. tx0+TX+1); windows anchored at
  // (ty0-2 .. ty0+TY-1) x (tx0-2 .. tx0+TX-1)
  __shared__ float dx_[TY + 4][TX + 5];
  __shared__ float dy_[TY + 4][TX + 5];
  __shared__ float wa[TY + 2][TX + 3];
  __shared__ float wb[TY + 2][TX + 3];
  __shared__ float wc[TY + 2][TX + 3];
  int btx_, bty_, b;
  if (!af_tile_of_block((W + TX - 1) / TX, (H + TY - 1) / TY, nimg, btx_, bty_, b)) return;
  const int ty0 = bty_ * TY, tx0 = btx_ * TX;
  const long cs = (long)H * W;
  const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
  const int x = tx0 + lx, y = ty0 + ly;
  const float c_l1 = coef[0], c_ss = coef[1];
  for (int c = 0; c < C; ++c) {
    const float* imc = im + ((long)b * C + c) * cs;
    const float* rc = rec + ((long)b * C + c) * cs;
    __syncthreads();
    for (int idx = threadIdx.x; idx < (TY + 4) * (TX + 4); idx += TX * TY) {
      const int r = idx / (TX + 4), cc = idx - r * (TX + 4);
      const int gy = ty0 + r - 2, gx = tx0 + cc - 2;
      float a = 0.f, bb = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long o = (long)gy * W + gx;
        const float m = mask ? mask[(long)b * cs + o] : 1.f;
        a = rc[o] * m;
        bb = imc[o] * m;
      }
      dx_[r][cc] = a;
      dy_[r][cc] = bb;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (TY + 2) * (TX + 2); idx += TX * TY) {
      const int r = idx / (TX + 2), cc = idx - r * (TX + 2);
      const int wy = ty0 + r - 2, wx = tx0 + cc - 2;  // window anchor
      float A = 0.f, Bc = 0.f, Cc = 0.f;
      if (wy >= 0 && wy < H - 2 && wx >= 0 && wx < W - 2)
        ssim_dist_grad(
            window_stats<TX + 5>(dx_, dy_, r, cc),
            [&] { return gmap ? gmap[(((long)b * C + c) * (H - 2) + wy) * (W - 2) + wx] : c_ss; }, A, Bc, Cc);
      wa[r][cc] = A;
      wb[r][cc] = Bc;
      wc[r][cc] = Cc;
    }
    __syncthreads();
    if (x < W && y < H) {
      Coef s;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)  // window anchored at (y-i, x-j) = tile slot (ly+2-i, lx+2-j)
          s.add(wa[ly + 2 - i][lx + 2 - j], wb[ly + 2 - i][lx + 2 - j], wc[ly + 2 - i][lx + 2 - j]);
      const long o = (long)y * W + x;
      const float m = mask ? mask[(long)b * cs + o] : 1.f;
      g_rec[((long)b * C + c) * cs + o] = rec_grad(m, c_l1, rc[o], imc[o], s, dx_[ly + 2][lx + 2], dy_[ly + 2][lx + 2]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// SSIM + L1, 4 pixels per lane (rows 16-byte aligned: W % 4 == 0).  The 1-px kernels above spend their time
// on scalar LDS reads (18 per window, 27 more per pixel in the backward): here a 16 x 64 pixel tile is
// staged with float4 loads (all in flight, none branched around), a lane owns 4 consecutive pixels and
// reads each window row as ds_read_b128 + ds_read_b64 (6 values serve its 4 windows).  Same arithmetic, in
// the same order, as the 1-px kernels (which remain for unaligned widths).
// ------------------------------------------------------------------------------------------------
namespace photo4 {
constexpr int P = 128;
// masked tiles x = recons*mask, y = im*mask: `rows` x `nq` float4 starting at image (gy0, gx0) (gx0 % 4 == 0)
template <int ROWS, int NQ, bool L1>
__device__ __forceinline__ float stage(float* __restrict__ X, float* __restrict__ Y, const float* __restrict__ imc,
                                       const float* __restrict__ rc, const float* __restrict__ mb, int H, int W,
                                       int gy0, int gx0, int own_r0, int own_q0) {
  constexpr int NS = ROWS * NQ, ITER = (NS + NT - 1) / NT;
  float4 iv[ITER], rv[ITER], mv[ITER];
  int r[ITER], q[ITER];
  bool ok[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int s = threadIdx.x + it * NT;
    r[it] = s / NQ, q[it] = s - r[it] * NQ;
    const int gy = gy0 + r[it], gx = gx0 + 4 * q[it];
    ok[it] = s < NS && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const long o = ok[it] ? (long)gy * W + gx : 0;
    iv[it] = *reinterpret_cast<const float4*>(imc + o);
    rv[it] = *reinterpret_cast<const float4*>(rc + o);
    mv[it] = mb ? *reinterpret_cast<const float4*>(mb + o) : make_float4(1.f, 1.f, 1.f, 1.f);
  }
  float l1 = 0.f;
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    if (threadIdx.x + it * NT < NS) {
      const float4 i4 = iv[it], r4 = rv[it], m4 = mv[it];
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(X + r[it] * P + 4 * q[it]) =
          ok[it] ? make_float4(r4.x * m4.x, r4.y * m4.y, r4.z * m4.z, r4.w * m4.w) : z;
      *reinterpret_cast<float4*>(Y + r[it] * P + 4 * q[it]) =
          ok[it] ? make_float4(i4.x * m4.x, i4.y * m4.y, i4.z * m4.z, i4.w * m4.w) : z;
      if (L1 && ok[it] && r[it] >= own_r0 && r[it] < own_r0 + TYH && q[it] >= own_q0 && q[it] < own_q0 + TXW / 4)
        l1 += ((fabsf(i4.x - r4.x) * m4.x + fabsf(i4.y - r4.y) * m4.y) + fabsf(i4.z - r4.z) * m4.z) +
              fabsf(i4.w - r4.w) * m4.w;
    }
  }
  return l1;
}

__global__ __launch_bounds__(NT) void fwd_kernel(const float* __restrict__ im, const float* __restrict__ rec,
                                                 const float* __restrict__ mask, float* __restrict__ ssim_map,
                                                 float* __restrict__ sums, int nrows, int nimg, int C, int H, int W) {
  __shared__ __attribute__((aligned(16))) float X[(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float Y[(TYH + 2) * P];
  __shared__ float red[3 * (NT / 64)];
  int btx, bty, b;
  if (!af_tile_of_block((W + TXW - 1) / TXW, (H + TYH - 1) / TYH, nimg, btx, bty, b)) {
    if (threadIdx.x == 0) af_store_partial(sums, nrows, 0.f, 0.f, 0.f);  // padding workgroup: its row must be defined
    return;
  }
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)H * W;
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  const float* mb = mask ? mask + (long)b * cs : nullptr;
  float part[3] = {0.f, 0.f, 0.f};
  if (y < H && x0 < W) {
    if (mb) {
      const float4 m = *reinterpret_cast<const float4*>(mb + (long)y * W + x0);
      part[2] = (m.x + m.y) + (m.z + m.w);
    } else {
      part[2] = 4.f;
    }
  }
  for (int c = 0; c < C; ++c) {
    if (c) __syncthreads();
    part[0] += stage<TYH + 2, TXW / 4 + 1, true>(X, Y, im + ((long)b * C + c) * cs, rec + ((long)b * C + c) * cs, mb, H,
                                                  W, ty0, tx0, 0, 0);
    __syncthreads();
    if (y < H - 2)
      fwd_windows<P>(X, Y, ly, xg, x0, W, [&](int e, float dist) {
        part[1] += dist;
        if (ssim_map) ssim_map[(((long)b * C + c) * (H - 2) + y) * (W - 2) + x0 + e] = dist;
      });
  }
  af_block_sum<3>(part, red);
  if (threadIdx.x == 0) af_store_partial(sums, nrows, part[0], part[1], part[2]);
}

__global__ __launch_bounds__(NT) void bwd_kernel(const float* __restrict__ im, const float* __restrict__ rec,
                                                 const float* __restrict__ mask, const float* __restrict__ gmap,
                                                 const float* __restrict__ coef, float* __restrict__ g_rec, int nimg,
                                                 int C, int H, int W) {
  // tile coordinates: row r <-> image row ty0 - 2 + r (20 rows), column q <-> image column tx0 - 4 + q (72);
  // window anchors live at rows 0..17, columns 2..65 of the same coordinates
  __shared__ __attribute__((aligned(16))) float X[(TYH + 4) * P];
  __shared__ __attribute__((aligned(16))) float Y[(TYH + 4) * P];
  __shared__ __attribute__((aligned(16))) float WA[(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float WB[(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float WC[(TYH + 2) * P];
  int btx, bty, b;
  if (!af_tile_of_block((W + TXW - 1) / TXW, (H + TYH - 1) / TYH, nimg, btx, bty, b)) return;
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)H * W;
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  const float* mb = mask ? mask + (long)b * cs : nullptr;
  const float c_l1 = coef[0], c_ss = coef[1];
  for (int c = 0; c < C; ++c) {
    const float* imc = im + ((long)b * C + c) * cs;
    const float* rc = rec + ((long)b * C + c) * cs;
    if (c) __syncthreads();
    stage<TYH + 4, TXW / 4 + 2, false>(X, Y, imc, rc, mb, H, W, ty0 - 2, tx0 - 4, 0, 0);
    __syncthreads();
    coef_pass<P>(X, Y, WA, WB, WC, ty0, tx0, H, W, [&](int wy, int wx) {
      return gmap ? gmap[(((long)b * C + c) * (H - 2) + wy) * (W - 2) + wx] : c_ss;
    });
    __syncthreads();
    if (y < H && x0 < W) {
      const long o = (long)y * W + x0;
      const float4 i4 = *reinterpret_cast<const float4*>(imc + o), r4 = *reinterpret_cast<const float4*>(rc + o);
      const float4 m4 = mb ? *reinterpret_cast<const float4*>(mb + o) : make_float4(1.f, 1.f, 1.f, 1.f);
      const float iv[4] = {i4.x, i4.y, i4.z, i4.w}, rv[4] = {r4.x, r4.y, r4.z, r4.w}, mv[4] = {m4.x, m4.y, m4.z, m4.w};
      float out[4];
      gather4<P>(X, Y, WA, WB, WC, ly, xg, [&](int e, const Coef& s, float xv, float yv) {
        out[e] = rec_grad(mv[e], c_l1, rv[e], iv[e], s, xv, yv);
      });
      *reinterpret_cast<float4*>(g_rec + ((long)b * C + c) * cs + o) = make_float4(out[0], out[1], out[2], out[3]);
    }
  }
}
}  // namespace photo4

}  // namespace

// 16 x 64 tiles and 4 pixels per lane where the rows are 16-byte aligned, else 8 x 32 tiles and 1 pixel per lane;
// 256 threads either way
static_assert(TX * TY == photo4::NT, "both tilings launch photo4::NT threads");
static bool photo_four(int W) { return (W & 3) == 0; }
static dim3 grid1(int B, int H, int W) { return dim3(af_grid_for_tiles((long)af_cdiv(W, TX) * af_cdiv(H, TY) * B)); }
static dim3 grid4(int B, int H, int W) { return dim3(af_grid_for_tiles(photo4::tiles(B, H, W))); }
static int photo_check(const float* im, const float* recons, int B, int C, int H, int W) {
  AF_REQUIRE_PTR(im);
  AF_REQUIRE_PTR(recons);
  AF_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && B <= 65535, ARFLOW_ESHAPE);
  return ARFLOW_OK;
}

extern "C" int arflow_photo_fwd(const float* im, const float* recons, const float* mask, float* ssim_map,
                                float* sums, int B, int C, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(sums);
  const int rc = photo_check(im, recons, B, C, H, W);
  if (rc != ARFLOW_OK) return rc;
  const int nrows = af_sums_rows(B, H, W);
  const bool four = photo_four(W);
  hipLaunchKernelGGL(four ? photo4::fwd_kernel : photo_fwd_kernel, four ? grid4(B, H, W) : grid1(B, H, W), dim3(photo4::NT),
                     0, (hipStream_t)stream, im, recons, mask, ssim_map, sums, nrows, B, C, H, W);
  return af_launch_status();
}

extern "C" int arflow_photo_bwd(const float* im, const float* recons, const float* mask, const float* gmap,
                                const float* coef, float* g_recons, int B, int C, int H, int W,
                                arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(coef);
  AF_REQUIRE_PTR(g_recons);
  const int rc = photo_check(im, recons, B, C, H, W);
  if (rc != ARFLOW_OK) return rc;
  const bool four = photo_four(W);
  hipLaunchKernelGGL(four ? photo4::bwd_kernel : photo_bwd_kernel, four ? grid4(B, H, W) : grid1(B, H, W), dim3(photo4::NT),
                     0, (hipStream_t)stream, im, recons, mask, gmap, coef, g_recons, B, C, H, W);
  return af_launch_status();
}
