// Fused warp + mask + L1/SSIM pass of the pyramid losses (unFlowLoss, MvLoss) for gfx950, and the area pyramid that
// feeds it.  Per scale ONE forward launch returns, per sample group (direction / view),
//   sum |tgt - rec| * m,   sum SSIMdist(rec * m, tgt * m),   sum m        with rec = flow_warp(src, flow, pad)
// (losses/flow_loss.py:13-27, losses/loss_blocks.py:65-84, utils/warp_utils.py:83-90,119-134) and ONE backward launch
// writes d/d flow.  The warped image, the mask and the gradient of the warped image never exist in memory, and the
// images / flows are addressed in place (base + b * stride + g * half), so the ATen cat / roll / 1 - x / nearest-resize
// kernels of the composed path are gone.
//
// Per-pixel arithmetic is that of warp_fwd_kernel / warp_bwd_flow_kernel (taps.hpp) and of photo4::fwd_kernel /
// bwd_kernel, whose window, coefficient and gather stages (ssim_dev.hpp) run here unchanged: only the order of the
// final summation differs from the composed path.
//
// Tiling: 16 x 64 pixels / 256 threads as photo4.  Every slot of the tile + halo (1 px forward, 2 px backward) warps
// its own pixel straight from global memory (3-channel images: the four taps of neighbouring pixels share cache lines;
// a staged source window as in warp_fwd_kernel would need a box reduction and two more barriers per tile for data that
// is read once) and stores x = rec * m, y = tgt * m of all channels in LDS; a lane then owns 4 consecutive pixels and
// reads the window rows as ds_read_b128 + ds_read_b64 like photo4.
#include "common.hpp"
#include "taps.hpp"
#include "ssim_dev.hpp"

namespace {

namespace pw {
using photo4::NT;
using photo4::TXW;
using photo4::TYH;
constexpr int P = 72, CMAX = 3;

struct Args {
  const float* tgt;
  long tgt_bs, tgt_half;
  const float* src;
  long src_bs, src_half;
  const float* flow;
  long flow_bs, flow_half;
  const float* mask;  // unused for ARFLOW_PW_MASK_BORDER
  long mask_bs, mask_half;
  int mask_mode, mask_invert, mask_w, mask_fy, mask_fx;
  int B, G, C, H, W, pad;
};

struct Pixel {
  TapPlan p;
  Taps t;
  float m;
};

// taps and mask of pixel (y, x); fl / mk point to the sample's flow / mask plane
__device__ __forceinline__ Pixel pixel(const Args& a, const float* __restrict__ fl, const float* __restrict__ mk, int y,
                                       int x) {
  Pixel px;
  const long o = (long)y * a.W + x;
  const float u = fl[o], v = fl[(long)a.H * a.W + o];
  px.t = make_taps((float)x, (float)y, u, v, a.H, a.W, a.H, a.W, a.pad, true, ARFLOW_NORM_ARFLOW);
  px.p = plan_taps(px.t, a.H, a.W);
  float m;
  if (a.mask_mode == ARFLOW_PW_MASK_BORDER) {  // border_mask(flow): open interval
    const float cx = (float)x + u, cy = (float)y + v;
    m = (cx > 0.f && cx < (float)(a.W - 1) && cy > 0.f && cy < (float)(a.H - 1)) ? 1.f : 0.f;
  } else if (a.mask_mode == ARFLOW_PW_MASK_NEAREST) {  // F.interpolate(mode='nearest'), integer factors
    m = mk[(long)(y * a.mask_fy) * a.mask_w + x * a.mask_fx];
  } else {
    m = mk[o];
  }
  px.m = a.mask_invert ? 1.f - m : m;
  return px;
}

// the four taps of one source plane (0 outside the source); all four loads unconditional (offsets are clamped)
__device__ __forceinline__ void taps4(const float* __restrict__ s, const TapPlan& p, float (&v)[4]) {
  float a0 = s[p.o[0]], a1 = s[p.o[1]], a2 = s[p.o[2]], a3 = s[p.o[3]];
  asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
  const float a[4] = {a0, a1, a2, a3};
  tap_select(p, a, v);
}

__global__ __launch_bounds__(NT) void fwd_kernel(Args a, float* __restrict__ mask_out, float* __restrict__ rows) {
  // tile coordinates: row r <-> image row ty0 + r (18 rows), column q <-> image column tx0 + q (66 used)
  __shared__ __attribute__((aligned(16))) float X[CMAX][(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float Y[CMAX][(TYH + 2) * P];
  __shared__ float red[3 * (NT / 64)];
  const int ntx = (a.W + TXW - 1) / TXW, nty = (a.H + TYH - 1) / TYH;
  int btx, bty, n;
  if (!af_tile_of_block(ntx, nty, a.B * a.G, btx, bty, n)) return;  // the rows are indexed by TILE: nothing to define
  const int g = n / a.B, b = n - g * a.B;
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)a.H * a.W;
  const float* tg = a.tgt + b * a.tgt_bs + g * a.tgt_half;
  const float* sr = a.src + b * a.src_bs + g * a.src_half;
  const float* fl = a.flow + b * a.flow_bs + g * a.flow_half;
  const float* mk = a.mask ? a.mask + b * a.mask_bs + g * a.mask_half : nullptr;
  float part[3] = {0.f, 0.f, 0.f};
  constexpr int NQ = TXW + 2, NS = (TYH + 2) * NQ;
  for (int s = threadIdx.x; s < NS; s += NT) {
    const int r = s / NQ, q = s - r * NQ;
    const int gy = ty0 + r, gx = tx0 + q;
    float xv[CMAX] = {0.f, 0.f, 0.f}, yv[CMAX] = {0.f, 0.f, 0.f};
    if (gy < a.H && gx < a.W) {
      const Pixel px = pixel(a, fl, mk, gy, gx);
      const long o = (long)gy * a.W + gx;
      const bool own = r < TYH && q < TXW;  // each pixel is owned by exactly one tile slot
      float l1 = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < a.C) {
          float v[4];
          taps4(sr + c * cs, px.p, v);
          const float rec = tap_blend(px.p, v), iv = tg[c * cs + o];
          xv[c] = rec * px.m;
          yv[c] = iv * px.m;
          l1 += fabsf(iv - rec) * px.m;
        }
      }
      if (own) {
        part[0] += l1;
        part[2] += px.m;
        if (mask_out) mask_out[(long)n * cs + o] = px.m;
      }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) X[c][r * P + q] = xv[c], Y[c][r * P + q] = yv[c];
  }
  __syncthreads();
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  if (y < a.H - 2 && x0 < a.W - 2) {
    for (int c = 0; c < a.C; ++c)
      photo4::fwd_windows<P>(X[c], Y[c], ly, xg, x0, a.W, [&](int, float dist) { part[1] += dist; });
  }
  af_block_sum<3>(part, red);
  if (threadIdx.x == 0) {
    const long t = ((long)n * nty + bty) * ntx + btx;
    *reinterpret_cast<float4*>(rows + t * ARFLOW_SUM_COLS) = make_float4(part[0], part[1], part[2], 0.f);
  }
}

// gflow: the gradient of the tensor the flow came from, same addressing as the flow (b * flow_bs + g * gflow_half)
__global__ __launch_bounds__(NT) void bwd_kernel(Args a, const float* __restrict__ coef, float* __restrict__ gflow,
                                                 long gflow_bs, long gflow_half) {
  // tile coordinates: row r <-> image row ty0 - 2 + r (20 rows), column q <-> image column tx0 - 4 + q (72);
  // window anchors live at rows 0..17, columns 2..67 of the same coordinates (photo4::bwd_kernel's layout)
  __shared__ __attribute__((aligned(16))) float X[CMAX][(TYH + 4) * P];
  __shared__ __attribute__((aligned(16))) float Y[CMAX][(TYH + 4) * P];
  __shared__ __attribute__((aligned(16))) float WA[(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float WB[(TYH + 2) * P];
  __shared__ __attribute__((aligned(16))) float WC[(TYH + 2) * P];
  const int ntx = (a.W + TXW - 1) / TXW, nty = (a.H + TYH - 1) / TYH;
  int btx, bty, n;
  if (!af_tile_of_block(ntx, nty, a.B * a.G, btx, bty, n)) return;
  const int g = n / a.B, b = n - g * a.B;
  const int ty0 = bty * TYH, tx0 = btx * TXW;
  const long cs = (long)a.H * a.W;
  const float* tg = a.tgt + b * a.tgt_bs + g * a.tgt_half;
  const float* sr = a.src + b * a.src_bs + g * a.src_half;
  const float* fl = a.flow + b * a.flow_bs + g * a.flow_half;
  const float* mk = a.mask ? a.mask + b * a.mask_bs + g * a.mask_half : nullptr;
  const float c_l1 = coef[2 * g], c_ss = coef[2 * g + 1];
  constexpr int NS = (TYH + 4) * P;
  for (int s = threadIdx.x; s < NS; s += NT) {
    const int r = s / P, q = s - r * P;
    const int gy = ty0 - 2 + r, gx = tx0 - 4 + q;
    float xv[CMAX] = {0.f, 0.f, 0.f}, yv[CMAX] = {0.f, 0.f, 0.f};
    if (q >= 2 && q < TXW + 6 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {  // columns 0, 1, 70, 71: padding
      const Pixel px = pixel(a, fl, mk, gy, gx);
      const long o = (long)gy * a.W + gx;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < a.C) {
          float v[4];
          taps4(sr + c * cs, px.p, v);
          xv[c] = tap_blend(px.p, v) * px.m;
          yv[c] = tg[c * cs + o] * px.m;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) X[c][s] = xv[c], Y[c][s] = yv[c];
  }
  // the lane's own 4 pixels: taps and masks stay in registers over the channel loop
  const int xg = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x0 = tx0 + 4 * xg, y = ty0 + ly;
  Pixel px[4];
  bool in[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    in[e] = y < a.H && x0 + e < a.W;
    px[e] = pixel(a, fl, mk, in[e] ? y : 0, in[e] ? x0 + e : 0);
  }
  float gix[4] = {0.f, 0.f, 0.f, 0.f}, giy[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < a.C; ++c) {
    __syncthreads();  // X / Y staged (c = 0); the previous channel's WA / WB / WC consumed (c > 0)
    photo4::coef_pass<P>(X[c], Y[c], WA, WB, WC, ty0, tx0, a.H, a.W, [&](int, int) { return c_ss; });
    __syncthreads();
    photo4::gather4<P>(X[c], Y[c], WA, WB, WC, ly, xg, [&](int e, const Coef& s, float xv, float yv) {
      float v[4];
      taps4(sr + c * cs, px[e].p, v);
      const float rec = tap_blend(px[e].p, v);
      const float iv = tg[c * cs + (in[e] ? (long)y * a.W + x0 + e : 0)];
      // photo4::bwd_kernel's d / d rec, fed into warp_bwd_flow_kernel's d rec / d coordinate
      const float gr = rec_grad(px[e].m, c_l1, rec, iv, s, xv, yv);
      float sx, sy;
      tap_corner_grad(px[e].t, v, sx, sy);
      gix[e] = fmaf(gr, sx, gix[e]);
      giy[e] = fmaf(gr, sy, giy[e]);
    });
  }
  float* gf = gflow + b * gflow_bs + g * gflow_half + (long)y * a.W + x0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (in[e]) {
      gf[e] = gix[e] * px[e].t.dx;
      gf[cs + e] = giy[e] * px[e].t.dy;
    }
}
}  // namespace pw

// ------------------------------------------------------------------------------------------------
// Area pyramid: every F.interpolate(frames, (h, w), mode='area') copy the loss needs (integer factors) in one launch,
// each computed from the full-resolution pixels.  Blocks above 64 pixels: 64 consecutive lanes share one output pixel, lane j
// adds the block's elements j, j + 64, ... (<= 64 each at factor 64), then the lane partials meet in a shuffle tree -- no
// fp32 running sum over more than 64 terms.  Smaller blocks: one lane each, see lanes_for().
// ------------------------------------------------------------------------------------------------
namespace ap {
constexpr int MAXL = ARFLOW_AREA_PYRAMID_MAX, NT = 256;
struct Level {
  int h, w, fy, fx, lanes;
  long out_off;    // floats from `out`
  long first_blk;  // first workgroup of this level
};
struct Args {
  int n, planes, H, W;
  Level lv[MAXL];
};

static inline int lanes_for(long block) {
  // up to 64 pixels (factors <= 8): one lane adds the block row by row, the order (and so the bits) of ATen's
  // adaptive average pooling on the GPU -- a scale computed here and one resized by F.interpolate see the same image
  if (block <= 64) return 1;
  int l = 1;
  while (l < 64 && l < block) l *= 2;
  return l;
}
static inline long blocks_for(long outputs, int lanes) { return (outputs * lanes + NT - 1) / NT; }

__global__ __launch_bounds__(NT) void kernel(Args a, const float* __restrict__ in, float* __restrict__ out) {
  int l = 0;
  while (l + 1 < a.n && (long)blockIdx.x >= a.lv[l + 1].first_blk) ++l;
  const Level lv = a.lv[l];
  const int L = lv.lanes;
  const long slot = ((long)blockIdx.x - lv.first_blk) * NT + threadIdx.x;
  const long o = slot / L;
  const int j = (int)(slot - o * L);
  const long nout = (long)a.planes * lv.h * lv.w;
  const bool ok = o < nout;  // (no early return: the shuffles below want every lane)
  float acc = 0.f;
  const int ox = (int)(o % lv.w), oy = (int)((o / lv.w) % lv.h);
  const long plane = o / ((long)lv.w * lv.h);
  if (ok) {
    const float* p = in + (plane * a.H + (long)oy * lv.fy) * a.W + (long)ox * lv.fx;
    const int nblk = lv.fy * lv.fx;
    for (int e = j; e < nblk; e += L) {
      const int r = e / lv.fx, c = e - r * lv.fx;
      acc += p[(long)r * a.W + c];
    }
  }
  for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, AF_WAVE);
  if (ok && j == 0) out[lv.out_off + o] = acc / (float)lv.fy / (float)lv.fx;
}
}  // namespace ap

int pw_validate(const pw::Args& a) {
  AF_REQUIRE_PTR(a.tgt);
  AF_REQUIRE_PTR(a.src);
  AF_REQUIRE_PTR(a.flow);
  AF_REQUIRE(a.B > 0 && a.G > 0 && a.C > 0 && a.H >= 3 && a.W >= 3 && (long)a.B * a.G <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE((long)a.H * a.W <= (1L << 30), ARFLOW_ESHAPE);
  AF_REQUIRE(a.C <= pw::CMAX, ARFLOW_EPARAM);
  AF_REQUIRE(a.pad == ARFLOW_PAD_ZEROS || a.pad == ARFLOW_PAD_BORDER, ARFLOW_EPARAM);
  AF_REQUIRE(a.mask_mode == ARFLOW_PW_MASK_PLANE || a.mask_mode == ARFLOW_PW_MASK_NEAREST ||
                 a.mask_mode == ARFLOW_PW_MASK_BORDER,
             ARFLOW_EPARAM);
  if (a.mask_mode != ARFLOW_PW_MASK_BORDER) AF_REQUIRE_PTR(a.mask);
  return ARFLOW_OK;
}

// mask_h / mask_w: extent of the fine plane of ARFLOW_PW_MASK_NEAREST (ignored by the other modes)
int pw_args(pw::Args& a, const float* tgt, long tgt_bs, long tgt_half, const float* src, long src_bs, long src_half,
            const float* flow, long flow_bs, long flow_half, const float* mask, long mask_bs, long mask_half, int mask_mode,
            int mask_invert, int mask_h, int mask_w, int B, int G, int C, int H, int W, int pad) {
  a.tgt = tgt, a.tgt_bs = tgt_bs, a.tgt_half = tgt_half;
  a.src = src, a.src_bs = src_bs, a.src_half = src_half;
  a.flow = flow, a.flow_bs = flow_bs, a.flow_half = flow_half;
  a.mask = mask_mode == ARFLOW_PW_MASK_BORDER ? nullptr : mask, a.mask_bs = mask_bs, a.mask_half = mask_half;
  a.mask_mode = mask_mode, a.mask_invert = mask_invert != 0, a.mask_w = W, a.mask_fy = 1, a.mask_fx = 1;
  a.B = B, a.G = G, a.C = C, a.H = H, a.W = W, a.pad = pad;
  const int rc = pw_validate(a);
  if (rc != ARFLOW_OK) return rc;
  if (mask_mode == ARFLOW_PW_MASK_NEAREST) {
    AF_REQUIRE(mask_h >= H && mask_w >= W && mask_h % H == 0 && mask_w % W == 0, ARFLOW_ESHAPE);
    a.mask_w = mask_w, a.mask_fy = mask_h / H, a.mask_fx = mask_w / W;
  }
  return ARFLOW_OK;
}

}  // namespace

extern "C" int arflow_photo_warp_rows(int N, int H, int W) {
  if (N <= 0 || H < 3 || W < 3) return ARFLOW_ESHAPE;
  const long t = photo4::tiles(N, H, W);
  return t > (1L << 30) ? ARFLOW_ESHAPE : (int)t;
}

extern "C" int arflow_photo_warp_fwd(const float* tgt, long tgt_bs, long tgt_half, const float* src, long src_bs,
                                     long src_half, const float* flow, long flow_bs, long flow_half, const float* mask,
                                     long mask_bs, long mask_half, int mask_mode, int mask_invert, int mask_h, int mask_w,
                                     float* mask_out, float* rows, int B, int G, int C, int H, int W, int pad_mode,
                                     arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(rows);
  pw::Args a;
  const int rc = pw_args(a, tgt, tgt_bs, tgt_half, src, src_bs, src_half, flow, flow_bs, flow_half, mask, mask_bs, mask_half,
                         mask_mode, mask_invert, mask_h, mask_w, B, G, C, H, W, pad_mode);
  if (rc != ARFLOW_OK) return rc;
  hipLaunchKernelGGL(pw::fwd_kernel, dim3(af_grid_for_tiles(photo4::tiles((long)B * G, H, W))), dim3(pw::NT), 0,
                     (hipStream_t)stream, a, mask_out, rows);
  return af_launch_status();
}

extern "C" int arflow_photo_warp_bwd(const float* tgt, long tgt_bs, long tgt_half, const float* src, long src_bs,
                                     long src_half, const float* flow, long flow_bs, long flow_half, const float* mask,
                                     long mask_bs, long mask_half, int mask_mode, int mask_invert, int mask_h, int mask_w,
                                     const float* coef, float* gflow, long gflow_bs, long gflow_half, int B, int G, int C,
                                     int H, int W, int pad_mode, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(coef);
  AF_REQUIRE_PTR(gflow);
  pw::Args a;
  const int rc = pw_args(a, tgt, tgt_bs, tgt_half, src, src_bs, src_half, flow, flow_bs, flow_half, mask, mask_bs, mask_half,
                         mask_mode, mask_invert, mask_h, mask_w, B, G, C, H, W, pad_mode);
  if (rc != ARFLOW_OK) return rc;
  hipLaunchKernelGGL(pw::bwd_kernel, dim3(af_grid_for_tiles(photo4::tiles((long)B * G, H, W))), dim3(pw::NT), 0,
                     (hipStream_t)stream, a, coef, gflow, gflow_bs, gflow_half);
  return af_launch_status();
}

// sizes: HOST array of n (h, w) pairs.  Returns the floats the packed output holds (>= 0) or an error.
static long ap_plan(ap::Args& a, int planes, int H, int W, const int* sizes, int n) {
  if (sizes == nullptr) return ARFLOW_ENULL;
  if (planes <= 0 || H <= 0 || W <= 0 || n <= 0) return ARFLOW_ESHAPE;
  if (n > ap::MAXL) return ARFLOW_EPARAM;
  a.n = 0, a.planes = planes, a.H = H, a.W = W;
  long off = 0, blk = 0;
  for (int i = 0; i < n; ++i) {
    const int h = sizes[2 * i], w = sizes[2 * i + 1];
    if (h <= 0 || w <= 0 || h > H || w > W || H % h != 0 || W % w != 0) return ARFLOW_ESHAPE;
    if (h == H && w == W) continue;  // factor 1: the frames themselves
    ap::Level& lv = a.lv[a.n++];
    lv.h = h, lv.w = w, lv.fy = H / h, lv.fx = W / w;
    lv.lanes = ap::lanes_for((long)lv.fy * lv.fx);
    lv.out_off = off, lv.first_blk = blk;
    off += (long)planes * h * w;
    blk += ap::blocks_for((long)planes * h * w, lv.lanes);
    if (blk > 0x7fffffffL || off > (1L << 40)) return ARFLOW_ESHAPE;
  }
  return off;
}

extern "C" long arflow_area_pyramid_ws_bytes(int planes, int H, int W, const int* sizes, int n) {
  ap::Args a;
  const long r = ap_plan(a, planes, H, W, sizes, n);
  return r < 0 ? r : r * (long)sizeof(float);
}

extern "C" int arflow_area_pyramid(const float* frames, float* out, int planes, int H, int W, const int* sizes, int n,
                                   arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(frames);
  ap::Args a;
  const long r = ap_plan(a, planes, H, W, sizes, n);
  if (r < 0) return (int)r;
  if (a.n == 0) return ARFLOW_OK;  // every size is the frames' own: nothing to produce
  AF_REQUIRE_PTR(out);
  const ap::Level& last = a.lv[a.n - 1];
  const long blocks = last.first_blk + ap::blocks_for((long)planes * last.h * last.w, last.lanes);
  hipLaunchKernelGGL(ap::kernel, dim3((unsigned)blocks), dim3(ap::NT), 0, (hipStream_t)stream, a, frames, out);
  return af_launch_status();
}
