// The augmentation-regularisation pass: the affine transform of an image stack, a flow field and a
// non-occlusion mask in ONE launch, and the masked robust loss between a prediction and the transformed flow.
//   theta [B][6] = (a b tx; c d ty) per sample, ON THE DEVICE: output pixel p' = (x', y') samples the source position
//                  s = (a x' + b y' + tx, c x' + d y' + ty), in pixel units;  d(p') = s - p',  L = [[a, b], [c, d]]
//   img_t  = flow_warp(img, d, pad='zeros', align_corners=True)     utils/warp_utils.py:83-90: bilinear, zero padding
//   g      = flow_warp(flow, d, pad='zeros');  flow_t = L^-1 g:  u_t = (d g_u - b g_v) / det,  v_t = (a g_v - c g_u) / det
//   mask_t = flow_warp(noc, d, pad='zeros') * border_mask(d)        utils/warp_utils.py:119-134: 0 < s_x < W - 1, 0 < s_y < H - 1,
//            strict; noc NULL reads as ones
// The sources are Hs x Ws planes and the destinations H x W planes (s and the border are the SOURCE's); the reference's
// functions are the case Hs = H, Ws = W, the other sizes carry a ground-truth flow through a crop or a resize.
// The fp32 operation order (no contraction, -ffp-contract=off; tests/ar_ref.py carries every step as value and bound):
//   s_x = (a x' + b y') + tx,  s_y = (c x' + d y') + ty;   x0 = floor(s_x), l1x = s_x - x0, l0x = 1 - l1x (same for y);
//   w00 = l0y l0x, w01 = l0y l1x, w10 = l1y l0x, w11 = l1y l1x, a tap outside the plane gets weight 0;
//   value = ((w00 p00 + w01 p01) + w10 p10) + w11 p11;   det = a d - b c;   the two quotients are IEEE divisions.
// s is formed directly: grid_sample's normalise / un-normalise round trip is not made.  s is clamped into [-2, Ws + 1] x
// [-2, Hs + 1] in front of floor (every tap is outside the plane beyond [-1, Ws] anyway, and a NaN becomes -2) and the tap
// indices are clamped into the plane before the address is formed: a theta nobody checked cannot make a lane read outside
// its plane.  border_mask uses the unclamped s.
// One lane owns four consecutive output x of one row: it computes s, the four taps and the four weights of each of its pixels
// ONCE and applies them to the C image channels, the two flow channels and the mask; rows are stored as float4 where
// W % 4 == 0 and the destinations are 16-byte aligned.
//
// The loss:  sums = { sum_{b,c,y,x} (|pred - flow_t| + eps)^q m,  sum_{b,y,x} m }   in float64 (m NULL reads as ones)
//   per element in fp32: e = pred - flow_t, t = |e| + eps, v = t (q == 1) or powf(t, q); the product v m and the sums in float64.
//   One workgroup takes 2048 pixels of one sample and stores ONE partial pair (af_block_sum_f64) into `work`
//   (arflow_ar_loss_partials pairs); a second launch of the same call adds the pairs in index order.  No atomics, no
//   zero-fill: two calls give the same bits, in either mode.
//   backward: gpred = ((k pw) m) sign(e),  k = (float)gsums[0] * q,  pw = 1 (q == 1) or powf(t, q - 1),  sign(0) = 0.
#include "common.hpp"

namespace {

constexpr int AR_NT = 256;
constexpr int AR_LOSS_PIX = 8;     // pixels per lane of the loss forward: 2048 per partial pair
constexpr int AR_FOLD_PAIRS = 512;  // partial pairs staged in LDS per trip of the fold
constexpr long AR_MAX_PLANE = 0x3fffffffL;
constexpr int AR_MAX_SIDE = 1 << 24;  // pixel indices are exact in fp32

struct ArArgs {
  const float* theta;
  const float* img;
  float* img_t;
  const float* flow;
  float* flow_t;
  const float* noc;
  float* mask_t;
  int B, C, Hs, Ws, H, W;  // source planes Hs x Ws, destination planes H x W
};

// the four taps of one output pixel: offsets inside a plane (clamped) and weights (0 for a tap outside the plane)
struct ArTaps {
  int i00, i01, i10, i11;
  float w00, w01, w10, w11;
};

__device__ __forceinline__ void ar_taps(float sx, float sy, int H, int W, ArTaps& t) {
  const float cx = fminf(fmaxf(sx, -2.0f), (float)W + 1.0f), cy = fminf(fmaxf(sy, -2.0f), (float)H + 1.0f);
  const float fx = floorf(cx), fy = floorf(cy);
  const float l1x = cx - fx, l1y = cy - fy;
  const float l0x = 1.0f - l1x, l0y = 1.0f - l1y;
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
  const int xa = min(max(x0, 0), W - 1), xb = min(max(x1, 0), W - 1);
  const int ra = min(max(y0, 0), H - 1) * W, rb = min(max(y1, 0), H - 1) * W;
  t.i00 = ra + xa, t.i01 = ra + xb, t.i10 = rb + xa, t.i11 = rb + xb;
  t.w00 = (vy0 && vx0) ? l0y * l0x : 0.f;
  t.w01 = (vy0 && vx1) ? l0y * l1x : 0.f;
  t.w10 = (vy1 && vx0) ? l1y * l0x : 0.f;
  t.w11 = (vy1 && vx1) ? l1y * l1x : 0.f;
}

__device__ __forceinline__ float ar_blend(const float* __restrict__ p, const ArTaps& t) {
  return ((t.w00 * p[t.i00] + t.w01 * p[t.i01]) + t.w10 * p[t.i10]) + t.w11 * p[t.i11];
}

template <bool VEC>
__global__ __launch_bounds__(AR_NT) void ar_transform_kernel(const ArArgs a) {
  const int b = blockIdx.y;
  const int wq = (a.W + 3) >> 2;
  const long q = (long)blockIdx.x * AR_NT + threadIdx.x;
  if (q >= (long)a.H * wq) return;
  const int y = (int)(q / wq), x0 = (int)(q % wq) * 4;
  const float* th = a.theta + b * 6;
  const float ta = th[0], tb = th[1], tx = th[2], tc = th[3], td = th[4], ty = th[5];
  const float by = tb * (float)y, dy = td * (float)y;
  ArTaps t[4];
  float inside[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // a column beyond W (scalar tail) computes clamped taps and stores nothing
    const float xf = (float)(x0 + j);
    const float sx = (ta * xf + by) + tx, sy = (tc * xf + dy) + ty;
    ar_taps(sx, sy, a.Hs, a.Ws, t[j]);
    inside[j] = (sx > 0.f && sx < (float)(a.Ws - 1) && sy > 0.f && sy < (float)(a.Hs - 1)) ? 1.f : 0.f;
  }
  const long hw = (long)a.H * a.W, shw = (long)a.Hs * a.Ws;
  const long row = (long)y * a.W;
  float v[4];
  if (a.img_t != nullptr) {
    for (int c = 0; c < a.C; ++c) {
      const long ch = (long)b * a.C + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ar_blend(a.img + ch * shw, t[j]);
      af_st_cols4<VEC>(a.img_t + ch * hw + row, x0, a.W, v);
    }
  }
  if (a.flow_t != nullptr) {
    const long plane = (long)b * 2 * hw, src = (long)b * 2 * shw;
    const float p1 = ta * td, p2 = tb * tc;
    const float det = p1 - p2;
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gu = ar_blend(a.flow + src, t[j]), gv = ar_blend(a.flow + src + shw, t[j]);
      u[j] = (td * gu - tb * gv) / det;
      v[j] = (ta * gv - tc * gu) / det;
    }
    af_st_cols4<VEC>(a.flow_t + plane + row, x0, a.W, u);
    af_st_cols4<VEC>(a.flow_t + plane + hw + row, x0, a.W, v);
  }
  if (a.mask_t != nullptr) {
    const long plane = (long)b * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m = a.noc != nullptr ? ar_blend(a.noc + b * shw, t[j]) : ((t[j].w00 + t[j].w01) + t[j].w10) + t[j].w11;
      v[j] = m * inside[j];
    }
    af_st_cols4<VEC>(a.mask_t + plane + row, x0, a.W, v);
  }
}

// |e| + eps, stated once: forward and backward must agree bit for bit
__device__ __forceinline__ float ar_base(float e, float eps) { return fabsf(e) + eps; }

__global__ __launch_bounds__(AR_NT) void ar_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ flow_t,
                                                            const float* __restrict__ mask, double* __restrict__ work, long hw,
                                                            float eps, float q) {
  __shared__ double scratch[2 * (AR_NT / AF_WAVE)];
  const int b = blockIdx.y;
  const float* pb = pred + (long)b * 2 * hw;
  const float* fb = flow_t + (long)b * 2 * hw;
  double acc[2] = {0.0, 0.0};
  for (int i = 0; i < AR_LOSS_PIX; ++i) {
    const long p = ((long)blockIdx.x * AR_LOSS_PIX + i) * AR_NT + threadIdx.x;
    if (p >= hw) break;
    const double m = mask != nullptr ? (double)mask[(long)b * hw + p] : 1.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float t = ar_base(pb[c * hw + p] - fb[c * hw + p], eps);
      const float v = q == 1.0f ? t : powf(t, q);
      acc[0] += (double)v * m;
    }
    acc[1] += m;
  }
  af_block_sum_f64<2, AR_NT>(acc, scratch);
  if (threadIdx.x == 0) {
    double* pair = work + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    pair[0] = acc[0], pair[1] = acc[1];
  }
}

// one workgroup: the n partial pairs are staged in LDS AR_FOLD_PAIRS at a time and added by lane 0 in index order
__global__ __launch_bounds__(AR_NT) void ar_loss_fold_kernel(const double* __restrict__ work, long n, double* __restrict__ sums) {
  __shared__ double stage[2 * AR_FOLD_PAIRS];
  double s0 = 0.0, s1 = 0.0;
  for (long base = 0; base < n; base += AR_FOLD_PAIRS) {
    const long left = n - base;
    const int cnt = (int)(left < AR_FOLD_PAIRS ? left : AR_FOLD_PAIRS);
    for (int i = threadIdx.x; i < 2 * cnt; i += AR_NT) stage[i] = work[base * 2 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < cnt; ++i) s0 += stage[2 * i], s1 += stage[2 * i + 1];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[0] = s0, sums[1] = s1;
}

__global__ __launch_bounds__(AR_NT) void ar_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ flow_t,
                                                            const float* __restrict__ mask, const double* __restrict__ gsums,
                                                            float* __restrict__ gpred, long hw, float eps, float q) {
  const long p = (long)blockIdx.x * AR_NT + threadIdx.x;
  if (p >= hw) return;
  const int b = blockIdx.y;
  const float k = (float)gsums[0] * q;
  const float m = mask != nullptr ? mask[(long)b * hw + p] : 1.0f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const long i = ((long)b * 2 + c) * hw + p;
    const float e = pred[i] - flow_t[i];
    const float pw = q == 1.0f ? 1.0f : powf(ar_base(e, eps), q - 1.0f);
    const float g = (k * pw) * m;
    gpred[i] = e > 0.f ? g : (e < 0.f ? -g : 0.f);
  }
}

inline long ar_loss_blocks(int H, int W) {
  const long per = (long)AR_NT * AR_LOSS_PIX;
  return ((long)H * W + per - 1) / per;
}

inline int ar_shape_check(int B, int H, int W) {
  AF_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= AR_MAX_SIDE && W <= AR_MAX_SIDE && (long)H * W <= AR_MAX_PLANE,
             ARFLOW_ESHAPE);
  return ARFLOW_OK;
}

// what the two loss launches share
inline int ar_loss_check(const float* pred, const float* flow_t, int B, int H, int W, float eps, float q) {
  AF_REQUIRE_PTR(pred);
  AF_REQUIRE_PTR(flow_t);
  const int rc = ar_shape_check(B, H, W);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(ar_loss_blocks(H, W) * B <= 0x7fffffffL, ARFLOW_ESHAPE);
  // the negations refuse a NaN; q < 1 at eps = 0 has an unbounded gradient where pred == flow_t
  AF_REQUIRE(eps >= 0.f && eps < INFINITY && q > 0.f && q < INFINITY && !(q < 1.0f && eps == 0.f), ARFLOW_EPARAM);
  return ARFLOW_OK;
}

}  // namespace

extern "C" int arflow_ar_transform(const float* theta, const float* img, float* img_t, int C, const float* flow, float* flow_t,
                                   const float* noc, float* mask_t, int B, int Hs, int Ws, int H, int W,
                                   arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(theta);
  if (img_t != nullptr) AF_REQUIRE_PTR(img);
  if (flow_t != nullptr) AF_REQUIRE_PTR(flow);
  AF_REQUIRE(img_t != nullptr || flow_t != nullptr || mask_t != nullptr, ARFLOW_EPARAM);
  int rc = ar_shape_check(B, H, W);
  if (rc == ARFLOW_OK) rc = ar_shape_check(B, Hs, Ws);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(img_t == nullptr || C >= 1, ARFLOW_ESHAPE);
  ArArgs a = {theta, img, img_t, flow, flow_t, noc, mask_t, B, C, Hs, Ws, H, W};
  // every plane is H W floats: with W % 4 == 0 an aligned base puts every row on a float4 boundary
  const bool vec = W % 4 == 0 && af_aligned16(img_t) && af_aligned16(flow_t) && af_aligned16(mask_t);
  const long nq = (long)H * ((W + 3) / 4);
  const dim3 grid((unsigned)((nq + AR_NT - 1) / AR_NT), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(ar_transform_kernel<true>, grid, dim3(AR_NT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ar_transform_kernel<false>, grid, dim3(AR_NT), 0, (hipStream_t)stream, a);
  return af_launch_status();
}

extern "C" int arflow_ar_loss_partials(int B, int H, int W) {
  const int rc = ar_shape_check(B, H, W);
  if (rc != ARFLOW_OK) return rc;
  const long n = ar_loss_blocks(H, W) * B;
  AF_REQUIRE(n <= 0x7fffffffL, ARFLOW_ESHAPE);
  return (int)n;
}

extern "C" int arflow_ar_loss_fwd(const float* pred, const float* flow_t, const float* mask, double* work, double* sums, int B,
                                  int H, int W, float eps, float q, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(work);
  AF_REQUIRE_PTR(sums);
  const int rc = ar_loss_check(pred, flow_t, B, H, W, eps, q);
  if (rc != ARFLOW_OK) return rc;
  const long nbx = ar_loss_blocks(H, W);
  hipLaunchKernelGGL(ar_loss_fwd_kernel, dim3((unsigned)nbx, (unsigned)B), dim3(AR_NT), 0, (hipStream_t)stream, pred, flow_t, mask,
                     work, (long)H * W, eps, q);
  AF_LAUNCH_CHECK();
  hipLaunchKernelGGL(ar_loss_fold_kernel, dim3(1), dim3(AR_NT), 0, (hipStream_t)stream, work, nbx * B, sums);
  return af_launch_status();
}

extern "C" int arflow_ar_loss_bwd(const float* pred, const float* flow_t, const float* mask, const double* gsums, float* gpred,
                                  int B, int H, int W, float eps, float q, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(gsums);
  AF_REQUIRE_PTR(gpred);
  const int rc = ar_loss_check(pred, flow_t, B, H, W, eps, q);
  if (rc != ARFLOW_OK) return rc;
  const long hw = (long)H * W;
  hipLaunchKernelGGL(ar_loss_bwd_kernel, dim3((unsigned)((hw + AR_NT - 1) / AR_NT), (unsigned)B), dim3(AR_NT), 0,
                     (hipStream_t)stream, pred, flow_t, mask, gsums, gpred, hw, eps, q);
  return af_launch_status();
}
