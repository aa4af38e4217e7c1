// The soft census arithmetic (utils/uflow_utils.py:213-293) of every kernel that computes it: the scalar and
// 4-pixels-per-lane kernels of photo.hip, census_any_* (generic.hip), the ordered (census_warp.hip), column
// (census_col.hpp / .hip) and pair-symmetric (census_sym.hip) families of the fused photometric direction.  One definition
// each, so that a fix reaches all of them and they agree bit for bit:
//   CENSUS_*, HAM_*, GRAY_*, GRAD_CONST     the constants
//   gray255                                 rgb_to_grayscale x 255 in the reference's operation order
//   pair_dist, pair_dist_acc, pair_grad     the pair term forward (plain / folded into a sum) and backward
//   pair_dist_acc_exact0                    the forward pair term that is exactly 0 for equal images (scalar kernel)
//   interior, ham_loss_terms                zero_mask_border and the census_loss epilogue of one pixel
//   flow_valid                              mask_invalid(flow_to_warp(flow))
//   Up4, up4_src, up4_coords, up4_clamped   upsample(clamp(range map, 0, 1), x4), torch bilinear, align_corners=False
//   dir_scale, store_dir_partial            pair mode: one scale / one pair of sums columns per direction
//   load_flow4, masked_loss4, corner_grads4 4 pixels per lane: flow vectors, the forward epilogue, (d sample / d flow)
//   store_rgb_grad, store_flow_grad         the backward's stores: d loss / d im_b and d loss / d flow
#pragma once
#include "common.hpp"
#include "taps.hpp"

namespace {

constexpr float CENSUS_EPS = 0.81f;  // t = d / sqrt(0.81 + d^2)
constexpr float CENSUS_THRESH = 0.1f;  // dist = sq / (0.1 + sq)
constexpr float HAM_EPS = 0.01f, HAM_POW = 0.4f, HAM_DPOW = -0.6f;  // abs_robust_loss: (|ham| + 0.01)^0.4, exponent - 1
constexpr float GRAY_R = 0.2989f, GRAY_G = 0.5870f, GRAY_B = 0.1140f;
// d dist / d sq = 0.1 q^2, d sq / d t_b = -2 e, d t_b / d d_b = 0.81 ub^3: the constants pair_grad leaves out
constexpr float GRAD_CONST = 0.1f * -2.f * 0.81f;

// ((r*0.2989 + g*0.5870) + b*0.1140) * 255, the reference's operation order
__device__ __forceinline__ float gray255(float r, float g, float b) {
  return ((r * GRAY_R + g * GRAY_G) + b * GRAY_B) * 255.f;
}
__device__ __forceinline__ float4 gray255(const float4& r, const float4& g, const float4& b) {
  return make_float4(gray255(r.x, g.x, b.x), gray255(r.y, g.y, b.y), gray255(r.z, g.z, b.z), gray255(r.w, g.w, b.w));
}

// soft census distance of one pixel pair: (t_a - t_b)^2 / (0.1 + (t_a - t_b)^2), t = d / sqrt(0.81 + d^2).
// pair_sq is its (t_a - t_b)^2; pair_dist_acc folds the quotient into a running sum as one FMA (the ordered kernels;
// in the column kernel that fold measured slower: forward 81 -> 84 us).
__device__ __forceinline__ float pair_sq(float ac, float bc, float an, float bn) {
  const float da = an - ac, db = bn - bc;
  const float tb = db * __builtin_amdgcn_rsqf(fmaf(db, db, CENSUS_EPS));
  const float e = fmaf(da, __builtin_amdgcn_rsqf(fmaf(da, da, CENSUS_EPS)), -tb);
  return e * e;
}
__device__ __forceinline__ float pair_dist(float ac, float bc, float an, float bn) {
  const float sq = pair_sq(ac, bc, an, bn);
  return sq * __builtin_amdgcn_rcpf(CENSUS_THRESH + sq);
}
__device__ __forceinline__ float pair_dist_acc(float ac, float bc, float an, float bn, float s) {
  const float sq = pair_sq(ac, bc, an, bn);
  return fmaf(sq, __builtin_amdgcn_rcpf(CENSUS_THRESH + sq), s);
}
// The same sum with both transforms rounded alike (two multiplications, no FMA between them): a pair whose grey differences
// agree in the two images contributes EXACTLY 0, so the distance of an image to itself is 0 even in the zero padding.  The
// scalar 32 x 8 forward (photo.hip, W % 4 != 0) keeps this form -- tests/test_census_gpu.py pins that zero through it.
__device__ __forceinline__ float pair_dist_acc_exact0(float ac, float bc, float an, float bn, float s) {
  const float da = an - ac, db = bn - bc;
  const float ta = da * __builtin_amdgcn_rsqf(fmaf(da, da, CENSUS_EPS));
  const float tb = db * __builtin_amdgcn_rsqf(fmaf(db, db, CENSUS_EPS));
  const float e = ta - tb, sq = e * e;
  return fmaf(sq, __builtin_amdgcn_rcpf(CENSUS_THRESH + sq), s);
}
// its derivative w.r.t. the grey value of image b at the FIRST pixel, before GRAD_CONST; odd under exchange of the two
// pixels
__device__ __forceinline__ float pair_grad(float ac, float bc, float an, float bn) {
  const float da = ac - an, db = bc - bn;
  const float ua = __builtin_amdgcn_rsqf(fmaf(da, da, CENSUS_EPS));
  const float ub = __builtin_amdgcn_rsqf(fmaf(db, db, CENSUS_EPS));
  const float e = fmaf(da, ua, -(db * ub));
  const float q = __builtin_amdgcn_rcpf(fmaf(e, e, CENSUS_THRESH));
  const float w = q * ub;  // q^2 e ub^3 = (q ub)^2 (e ub): 4 multiplications instead of 5
  return (w * w) * (e * ub);
}

// zero_mask_border (utils/uflow_utils.py:234-238)
__device__ __forceinline__ bool interior(int y, int x, int H, int W, int R) {
  return y >= R && y < H - R && x >= R && x < W - R;
}
// census_loss of one pixel with soft distance s and border-zeroed mask pm: adds (|s| + 0.01)^0.4 pm and pm to the two
// partial sums; dh = d / d s of the first
__device__ __forceinline__ void ham_loss_terms(float s, float pm, float (&part)[2], float& dh) {
  const float lg = __log2f(fabsf(s) + HAM_EPS);
  part[0] += exp2f(HAM_POW * lg) * pm;
  part[1] += pm;
  dh = pm * HAM_POW * exp2f(HAM_DPOW * lg);
}

// mask_invalid(flow_to_warp(flow)), utils/uflow_utils.py:35-50 (as warp_fwd_kernel's `valid`)
__device__ __forceinline__ float flow_valid(int x, int y, float u, float v, int H, int W) {
  const float cx = (float)x + u, cy = (float)y + v;
  return (cx >= 0.f && cx <= (float)(W - 1) && cy >= 0.f && cy <= (float)(H - 1)) ? 1.f : 0.f;
}

// x4 bilinear upsampling of a [h, w] plane, torch's arithmetic (align_corners=False): source position of output index p,
// the four cells and the two weights of output pixel (y, x), and the blend
__device__ __forceinline__ float up4_src(int p) { return fmaxf(0.25f * ((float)p + 0.5f) - 0.5f, 0.f); }
struct Up4 {
  int ya, xa, yb, xb;
  float ly, lx;
  __device__ __forceinline__ float blend(float v00, float v01, float v10, float v11) const {
    return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
};
__device__ __forceinline__ Up4 up4_coords(int h, int w, int y, int x) {
  const float sy = up4_src(y), sx = up4_src(x);
  Up4 c;
  c.ya = (int)sy, c.xa = (int)sx;
  c.yb = c.ya + (c.ya < h - 1 ? 1 : 0), c.xb = c.xa + (c.xa < w - 1 ? 1 : 0);
  c.ly = sy - (float)c.ya, c.lx = sx - (float)c.xa;
  return c;
}
// upsample(clamp(occ, 0, 1), x4)[y, x] (as up4_clamp_mul_kernel, smooth.hip)
__device__ __forceinline__ float up4_clamped(const float* __restrict__ occ, int h, int w, int y, int x) {
  const Up4 c = up4_coords(h, w, y, x);
  auto cl = [](float v) { return fminf(fmaxf(v, 0.f), 1.f); };
  return c.blend(cl(occ[(long)c.ya * w + c.xa]), cl(occ[(long)c.ya * w + c.xb]), cl(occ[(long)c.yb * w + c.xa]),
                 cl(occ[(long)c.yb * w + c.xb]));
}

// Pair mode: the batch interleaves the two directions of UFlowLoss (sample s = 2 b + direction), with one backward scale
// per direction and the partial sums of direction 1 in columns (2, 3) of the row instead of (0, 1).
__device__ __forceinline__ float dir_scale(const float* scale, int pair, int b) {
  return (scale ? scale[pair ? (b & 1) : 0] : 1.f) * GRAD_CONST;
}
__device__ __forceinline__ void store_dir_partial(float* __restrict__ sums, int nrows, const float (&part)[2], int pair,
                                                  int b) {
  const bool dir1 = pair && (b & 1);
  af_store_partial(sums, nrows, dir1 ? 0.f : part[0], dir1 ? 0.f : part[1], dir1 ? part[0] : 0.f, dir1 ? part[1] : 0.f);
}

// the flow vectors of 4 consecutive pixels at plane offset o (W % 4 == 0: aligned)
__device__ __forceinline__ void load_flow4(const float* __restrict__ fl, long cs, long o, float (&u)[4], float (&v)[4]) {
  const float4 fu = *reinterpret_cast<const float4*>(fl + o);
  const float4 fv = *reinterpret_cast<const float4*>(fl + cs + o);
  u[0] = fu.x, u[1] = fu.y, u[2] = fu.z, u[3] = fu.w;
  v[0] = fv.x, v[1] = fv.y, v[2] = fv.z, v[3] = fv.w;
}
// The forward epilogue of the 4-pixels-per-lane fused kernels for pixels (x0 .. x0 + 3, y) with soft distances s:
// mv = mask_invalid x the upsampled range map (occ nullable), the loss terms of ham_loss_terms under the border-zeroed mask
__device__ __forceinline__ void masked_loss4(const float* __restrict__ fl, const float* __restrict__ occ, const float (&s)[4],
                                             int x0, int y, int H, int W, int R, float (&mv)[4], float (&dh)[4],
                                             float (&part)[2]) {
  float uu[4], vv[4];
  load_flow4(fl, (long)H * W, (long)y * W + x0, uu, vv);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float val = flow_valid(x0 + p, y, uu[p], vv[p], H, W);
    mv[p] = occ ? up4_clamped(occ, H / 4, W / 4, y, x0 + p) * val : val;
    ham_loss_terms(s[p], interior(y, x0 + p, H, W, R) ? mv[p] : 0.f, part, dh[p]);
  }
}
// (d sample / d coordinate) * (d coordinate / d flow) of the warp at pixels (x0 .. x0 + 3, y): the bilinear corner
// differences of the grey plane sb
__device__ __forceinline__ void corner_grads4(const float* __restrict__ sb, const float* __restrict__ fl, int x0, int y,
                                              int H, int W, float (&cdx)[4], float (&cdy)[4]) {
  float uu[4], vv[4];
  load_flow4(fl, (long)H * W, (long)y * W + x0, uu, vv);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const Taps t = make_taps((float)(x0 + p), (float)y, uu[p], vv[p], H, W, H, W, ARFLOW_PAD_ZEROS, true, ARFLOW_NORM_UFLOW);
    const TapPlan pl = plan_taps(t, H, W);
    float a[4], sx, sy;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = sb[pl.o[q]];
    tap_select(pl, a, a);
    tap_corner_grad(t, a, sx, sy);
    cdx[p] = sx * t.dx;
    cdy[p] = sy * t.dy;
  }
}

// N = 1 or 4 consecutive pixels of one row; N = 4 stores float4 (aligned)
template <int N>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[N]) {
  static_assert(N == 1 || N == 4, "one pixel or an aligned group of four");
  if constexpr (N == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}
// d loss / d im_b = sc * acc * the colour weights (sc carries the x255 of the grey plane); o: the red plane's pixel
template <int N>
__device__ __forceinline__ void store_rgb_grad(float* __restrict__ o, long cs, float sc, const float (&acc)[N]) {
  const float wgt[3] = {GRAY_R, GRAY_G, GRAY_B};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[N];
#pragma unroll
    for (int p = 0; p < N; ++p) v[p] = sc * acc[p] * wgt[c];
    store_row<N>(o + c * cs, v);
  }
}
// d loss / d flow = sc * acc * the warp's flow gradient; gf: the x plane's pixel
template <int N>
__device__ __forceinline__ void store_flow_grad(float* __restrict__ gf, long cs, float sc, const float (&acc)[N],
                                                const float (&cdx)[N], const float (&cdy)[N]) {
  float vx[N], vy[N];
#pragma unroll
  for (int p = 0; p < N; ++p) vx[p] = sc * acc[p] * cdx[p], vy[p] = sc * acc[p] * cdy[p];
  store_row<N>(gf, vx);
  store_row<N>(gf + cs, vy);
}

}  // namespace
