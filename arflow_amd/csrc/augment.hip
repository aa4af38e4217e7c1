// On-device batch augmentation: the raw batch src [B][F][3][Hs][Ws] (uint8, or float32 already in
// [0,1]) is read ONCE and both float32 versions the trainer needs (trainer/uflow_trainer.py:35-54) are stored, in the
// channel-concatenated layout [B][3F][h][w]:   img = geometric only,   img_ph = geometric + photometric (may be NULL).
//   geometric    transforms/geometric_transforms.py:7-15: crop (y1, x1, th, tw) -> hflip -> optional bilinear resize of the
//                cropped, flipped image to (h, w), align_corners = False (rf_axis of resize_dev.hpp, the blend in ATen's order).
//                Without the resize (h, w) = (th, tw) and img is src / 255 (ONE IEEE division) at the mapped pixel, bit for bit.
//   photometric  transforms/photometric_transforms.py:7-25: ColorJitter's four operations in the sample's order, each ending
//                in a clamp to [0,1], then gamma, then the channel permutation.  The arithmetic is the tensor path of
//                torchvision.transforms.functional, restated from its published formulas (ag_* below); inactive operations
//                are skipped, not applied with an identity factor.
// Every frame of a sample shares the sample's row of the parameter table (include/arflow_hip.h: ARFLOW_AUG_*).
// Contrast blends with the frame's mean grey AS THE FRAME STANDS WHEN CONTRAST'S TURN COMES: arflow_augment_stats applies the
// operations in front of contrast, sums grey in float64 (af_block_sum_f64) and stores ONE partial per workgroup; the apply
// kernel adds a frame's partials in index order.  No atomics, no zero-fill: two calls give the same bits, in either mode.
// One lane owns four consecutive output x of one frame and all three channels (hue, saturation and the permutation need them
// together); the six output rows it stores are float4 where w % 4 == 0 and the outputs are 16-byte aligned.
#include "common.hpp"
#include "resize_dev.hpp"

namespace {

constexpr int AG_NT = 256;
constexpr int AG_STAT_QUADS = 2;  // quads of four pixels per lane of the stats kernel: 2048 pixels per partial
constexpr long AG_MAX_PLANE = 0x3fffffffL;
constexpr int AG_BRIGHTNESS = 0, AG_CONTRAST = 1, AG_SATURATION = 2, AG_HUE = 3;

struct AgArgs {
  const void* src;
  const int* tab;
  double* part;  // [B F][nparts]
  float* img;
  float* img_ph;
  int B, F, Hs, Ws, th, tw, h, w, scale, nparts;
};

// a sample's row of the table, as the kernels use it
struct AgRow {
  int y1, x1, flags, order, perm;
  float factor[4], gamma;
};

__device__ __forceinline__ AgRow ag_row(const AgArgs& a, int b) {
  const int* t = a.tab + (long)b * ARFLOW_AUG_ROW;
  AgRow r;
  // the window is clamped into the source: a table the host did not check cannot make a lane read outside src
  r.y1 = min(max(t[ARFLOW_AUG_Y1], 0), a.Hs - a.th);
  r.x1 = min(max(t[ARFLOW_AUG_X1], 0), a.Ws - a.tw);
  r.flags = t[ARFLOW_AUG_FLAGS];
  r.order = t[ARFLOW_AUG_ORDER];
  r.perm = t[ARFLOW_AUG_PERM];
#pragma unroll
  for (int k = 0; k < 4; ++k) r.factor[k] = __int_as_float(t[ARFLOW_AUG_FACTOR + k]);
  r.gamma = __int_as_float(t[ARFLOW_AUG_GAMMA]);
  return r;
}

__device__ __forceinline__ bool ag_active(const AgRow& r, int op) { return (r.flags >> (1 + op)) & 1; }
// by selects: a dynamic index would move the row out of registers
__device__ __forceinline__ float ag_factor(const AgRow& r, int op) {
  return op == 0 ? r.factor[0] : (op == 1 ? r.factor[1] : (op == 2 ? r.factor[2] : r.factor[3]));
}

__device__ __forceinline__ float ag_value(const uint8_t* p) { return (float)*p / 255.0f; }
__device__ __forceinline__ float ag_value(const float* p) { return *p; }

// the geometric stage for one output pixel (y, x) of one frame -> the three channels
template <typename T>
__device__ __forceinline__ void ag_fetch(const T* __restrict__ frame, const AgArgs& a, const AgRow& r, int y, int x, float (&c)[3]) {
  const long plane = (long)a.Hs * a.Ws;
  const bool flip = r.flags & ARFLOW_AUG_FLIP;
  if (!a.scale) {
    const T* p = frame + (long)(r.y1 + y) * a.Ws + r.x1 + (flip ? a.tw - 1 - x : x);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = ag_value(p + ch * plane);
    return;
  }
  const RfAxis ay = rf_axis(y, a.th, a.h, 0), ax = rf_axis(x, a.tw, a.w, 0);
  const int xa = r.x1 + (flip ? a.tw - 1 - ax.i0 : ax.i0), xb = r.x1 + (flip ? a.tw - 1 - ax.i1 : ax.i1);
  const T* r0 = frame + (long)(r.y1 + ay.i0) * a.Ws;
  const T* r1 = frame + (long)(r.y1 + ay.i1) * a.Ws;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float top = ax.l0 * ag_value(r0 + ch * plane + xa) + ax.l1 * ag_value(r0 + ch * plane + xb);
    const float bot = ax.l0 * ag_value(r1 + ch * plane + xa) + ax.l1 * ag_value(r1 + ch * plane + xb);
    c[ch] = ay.l0 * top + ay.l1 * bot;
  }
}

__device__ __forceinline__ float ag_clamp(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float ag_gray(const float (&c)[3]) { return 0.2989f * c[0] + 0.587f * c[1] + 0.114f * c[2]; }
// clamp(f a + (1 - f) b, 0, 1)
__device__ __forceinline__ float ag_blend(float a, float b, float f) { return ag_clamp(f * a + (1.0f - f) * b); }

// the hexcone round trip with the hue moved by f
__device__ __forceinline__ void ag_hue(float (&c)[3], float f) {
  const float r = c[0], g = c[1], b = c[2];
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const float cr = maxc - minc;
  const bool eq = cr == 0.f;
  const float s = cr / (eq ? 1.0f : maxc);
  const float dv = eq ? 1.0f : cr;
  const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
  float hh;
  if (maxc == r)
    hh = bc - gc;
  else if (maxc == g)
    hh = (2.0f + rc) - bc;
  else
    hh = (4.0f + gc) - rc;
  hh = hh / 6.0f + 1.0f;
  hh = hh - floorf(hh);  // fmod(., 1) of a positive number
  hh = hh + f;
  hh = hh - floorf(hh);
  const float h6 = hh * 6.0f;
  const float fi = floorf(h6);
  const float ph = h6 - fi;
  const float v = maxc;
  const float p = ag_clamp(v * (1.0f - s));
  const float q = ag_clamp(v * (1.0f - s * ph));
  const float t = ag_clamp(v * (1.0f - s * (1.0f - ph)));
  switch ((int)fi % 6) {
    case 0: c[0] = v, c[1] = t, c[2] = p; break;
    case 1: c[0] = q, c[1] = v, c[2] = p; break;
    case 2: c[0] = p, c[1] = v, c[2] = t; break;
    case 3: c[0] = p, c[1] = q, c[2] = v; break;
    case 4: c[0] = t, c[1] = p, c[2] = v; break;
    default: c[0] = v, c[1] = p, c[2] = q; break;
  }
}

// one ColorJitter operation on one pixel; mean: the frame's mean grey (contrast only)
__device__ __forceinline__ void ag_jitter(int op, float f, float mean, float (&c)[3]) {
  if (op == AG_BRIGHTNESS) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = ag_clamp(f * c[ch]);
  } else if (op == AG_CONTRAST) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = ag_blend(c[ch], mean, f);
  } else if (op == AG_SATURATION) {
    const float gr = ag_gray(c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = ag_blend(c[ch], gr, f);
  } else if (op == AG_HUE) {
    ag_hue(c, f);
  }
}

__device__ __forceinline__ int ag_op_at(const AgRow& r, int k) { return (r.order >> (2 * k)) & 3; }

// partial sums of grey of frame blockIdx.y as it stands in front of contrast; nothing to do where contrast is inactive
template <typename T>
__global__ __launch_bounds__(AG_NT) void augment_stats_kernel(const AgArgs a) {
  __shared__ double scratch[AG_NT / AF_WAVE];
  const int bf = blockIdx.y, b = bf / a.F;
  const AgRow r = ag_row(a, b);
  if (!ag_active(r, AG_CONTRAST)) return;  // uniform over the workgroup
  const T* frame = (const T*)a.src + (long)bf * 3 * a.Hs * a.Ws;
  const int wq = (a.w + 3) >> 2;
  const long nq = (long)a.h * wq;
  double acc[1] = {0.0};
  for (int i = 0; i < AG_STAT_QUADS; ++i) {
    const long q = ((long)blockIdx.x * AG_STAT_QUADS + i) * AG_NT + threadIdx.x;
    if (q >= nq) break;
    const int y = (int)(q / wq), x0 = (int)(q % wq) * 4;
    for (int j = 0; j < 4 && x0 + j < a.w; ++j) {
      float c[3];
      ag_fetch(frame, a, r, y, x0 + j, c);
      for (int k = 0; k < 4; ++k) {
        const int op = ag_op_at(r, k);
        if (op == AG_CONTRAST) break;
        if (ag_active(r, op)) ag_jitter(op, ag_factor(r, op), 0.f, c);
      }
      acc[0] += (double)ag_gray(c);
    }
  }
  af_block_sum_f64<1, AG_NT>(acc, scratch);
  if (threadIdx.x == 0) a.part[(long)bf * a.nparts + blockIdx.x] = acc[0];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(AG_NT) void augment_apply_kernel(const AgArgs a) {
  __shared__ float mean_s;
  const int bf = blockIdx.y, b = bf / a.F, f = bf - b * a.F;
  const AgRow r = ag_row(a, b);
  const bool photo = a.img_ph != nullptr;
  if (photo && ag_active(r, AG_CONTRAST) && a.part != nullptr) {  // uniform over the workgroup
    if (threadIdx.x == 0) {
      const double* p = a.part + (long)bf * a.nparts;
      double s = 0.0;
      for (int i = 0; i < a.nparts; ++i) s += p[i];
      mean_s = (float)(s / (double)((long)a.h * a.w));
    }
    __syncthreads();
  }
  const int wq = (a.w + 3) >> 2;
  const long q = (long)blockIdx.x * AG_NT + threadIdx.x;
  if (q >= (long)a.h * wq) return;
  const float mean = (photo && ag_active(r, AG_CONTRAST) && a.part != nullptr) ? mean_s : 0.f;
  const int y = (int)(q / wq), x0 = (int)(q % wq) * 4;
  const T* frame = (const T*)a.src + (long)bf * 3 * a.Hs * a.Ws;
  float g[3][4], ph[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float c[3] = {0.f, 0.f, 0.f};
    if (x0 + j < a.w) ag_fetch(frame, a, r, y, x0 + j, c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g[ch][j] = c[ch];
    if (photo) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int op = ag_op_at(r, k);
        if (ag_active(r, op)) ag_jitter(op, ag_factor(r, op), mean, c);
      }
      if (r.flags & ARFLOW_AUG_GAMMA_ON) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ag_clamp(powf(c[ch], r.gamma));
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int from = (r.perm >> (2 * ch)) & 3;
        ph[ch][j] = from == 0 ? c[0] : (from == 1 ? c[1] : c[2]);
      }
    }
  }
  const long hw = (long)a.h * a.w;
  const long row = ((long)b * 3 * a.F + 3 * f) * hw + (long)y * a.w;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    af_st_cols4<VEC>(a.img + row + ch * hw, x0, a.w, g[ch]);
    if (photo) af_st_cols4<VEC>(a.img_ph + row + ch * hw, x0, a.w, ph[ch]);
  }
}

inline int ag_partials(int h, int w) {
  const long nq = (long)h * ((w + 3) / 4), per = (long)AG_NT * AG_STAT_QUADS;
  return (int)((nq + per - 1) / per);
}

// the arguments the two launches share -> the kernels' argument block
inline int ag_check(const void* src, int dtype, const int* tab, int B, int F, int Hs, int Ws, int th, int tw, int h, int w, int scale,
                    AgArgs& a) {
  AF_REQUIRE_PTR(src);
  AF_REQUIRE_PTR(tab);
  AF_REQUIRE(dtype == ARFLOW_AUG_U8 || dtype == ARFLOW_AUG_F32, ARFLOW_EPARAM);
  AF_REQUIRE(scale == 0 || scale == 1, ARFLOW_EPARAM);
  AF_REQUIRE(B >= 1 && F >= 1 && F <= ARFLOW_AUG_MAX_FRAMES && (long)B * F <= 65535, ARFLOW_ESHAPE);
  AF_REQUIRE(h >= 1 && w >= 1 && Hs >= 1 && Ws >= 1 && (long)h * w <= AG_MAX_PLANE && (long)Hs * Ws <= AG_MAX_PLANE, ARFLOW_ESHAPE);
  AF_REQUIRE(th >= 1 && tw >= 1 && th <= Hs && tw <= Ws, ARFLOW_ESHAPE);
  AF_REQUIRE(scale || (h == th && w == tw), ARFLOW_ESHAPE);
  a.src = src, a.tab = tab;
  a.B = B, a.F = F, a.Hs = Hs, a.Ws = Ws, a.th = th, a.tw = tw, a.h = h, a.w = w, a.scale = scale;
  a.nparts = ag_partials(h, w);
  return ARFLOW_OK;
}

}  // namespace

extern "C" int arflow_augment_partials(int h, int w) {
  AF_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= AG_MAX_PLANE, ARFLOW_ESHAPE);
  return ag_partials(h, w);
}

extern "C" int arflow_augment_stats(const void* src, int dtype, const int* table, double* work, int B, int F, int Hs, int Ws,
                                    int th, int tw, int h, int w, int scale, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(work);
  AgArgs a = {};
  const int rc = ag_check(src, dtype, table, B, F, Hs, Ws, th, tw, h, w, scale, a);
  if (rc != ARFLOW_OK) return rc;
  a.part = work;
  const dim3 grid((unsigned)a.nparts, (unsigned)(B * F));
  if (dtype == ARFLOW_AUG_U8)
    hipLaunchKernelGGL(augment_stats_kernel<uint8_t>, grid, dim3(AG_NT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(augment_stats_kernel<float>, grid, dim3(AG_NT), 0, (hipStream_t)stream, a);
  return af_launch_status();
}

extern "C" int arflow_augment_apply(const void* src, int dtype, const int* table, const double* work, float* img, float* img_ph,
                                    int B, int F, int Hs, int Ws, int th, int tw, int h, int w, int scale,
                                    arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(img);
  AgArgs a = {};
  const int rc = ag_check(src, dtype, table, B, F, Hs, Ws, th, tw, h, w, scale, a);
  if (rc != ARFLOW_OK) return rc;
  a.part = const_cast<double*>(work), a.img = img, a.img_ph = img_ph;
  const long hw = (long)h * w;
  const bool vec = w % 4 == 0 && af_vec4_ok(img, hw, 2) && af_vec4_ok(img_ph, hw, 2);
  const long nq = (long)h * ((w + 3) / 4);
  const dim3 grid((unsigned)((nq + AG_NT - 1) / AG_NT), (unsigned)(B * F));
  auto launch = [&](auto t) {
    using T = decltype(t);
    if (vec)
      hipLaunchKernelGGL((augment_apply_kernel<T, true>), grid, dim3(AG_NT), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL((augment_apply_kernel<T, false>), grid, dim3(AG_NT), 0, (hipStream_t)stream, a);
  };
  if (dtype == ARFLOW_AUG_U8)
    launch(uint8_t{});
  else
    launch(float{});
  return af_launch_status();
}
