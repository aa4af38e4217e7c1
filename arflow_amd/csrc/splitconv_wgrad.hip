// Weight gradient of the 3x3 convolution (stride 1, zero padding 1, dilation 1) of the WIDE layers on the bf16 matrix cores at
// fp32 accuracy, for gfx950 (forward and data gradient: splitconv.hip, section 17):
//
//     dW[k][c][r][s] = sum over (n, h, w) of dy[n][k][h][w] * x[n][c][h + r - 1][w + s - 1]          (zero outside the image)
//
// GEMM view, per tap: D[k][c] = sum over pixels of A[k][pixel] * B[pixel][c], A = dy, B = x shifted by the tap, the reduction
// over PIXELS -- which are contiguous per channel in NCHW, so nothing is transposed.  Both operands are split into their three
// bf16 planes in registers on the way to LDS (splitbf16.hpp, Split: b0 + b1 + b2 == x bit for bit) and the same six plane
// products are accumulated by v_mfma_f32_32x32x16_bf16, the three smallest dropped.
//
// Work split.  The map is cut into strips of at most 8 groups of 8 pixels (64 columns) and into blocks of rows; a CHUNK is
// (sample, strip, row block).  A workgroup owns one chunk, CT <= 2 tiles of 32 input channels and KT <= 2 tiles of 32 output
// channels, and walks down the chunk's rows.  Per row it stages the dy row (KT * 32 channels) and the
// NEXT x row (CT * 32 channels) as bf16 planes -- the x rows h - 1, h, h + 1 live in a ring of three -- with zero fill for
// rows outside the image, columns outside it, the groups past the strip, the channel tails and the tiles a part does not
// have; no global address is formed for any of them.  A lane's MFMA
// fragment is 8 consecutive pixels of one channel: one ds_read_b128.  The +-1 column taps are the same run shifted by ONE
// element, i.e. off the 16-byte boundary: instead of three copies in LDS, the two neighbours of every group (pixel 8g - 1 and
// 8g + 8, zero at the image's edge) are stored as one dword next to it and the shifted fragments are made in registers with
// five v_alignbit_b32 per plane.  Channel strides are an odd number of 16-byte slots (25 for dy, 73 for x), so the 16 lanes a
// ds_read_b128 phase serves fall on 16 different slots of the bank row.
// A wave is (output-channel tile, input-channel tile, tap row r): it reads dy row h and x row h + r - 1 and holds the three
// taps (r, 0..2) of its 32 x 32 tile: 48 accumulator registers for the current row plus 48 running totals.  3 KT CT waves per
// workgroup: at KT = CT = 2 twelve waves, three per SIMD (<= 168 registers), 116 KB of LDS, one workgroup per CU; a staged
// dy row then serves two x tiles and a staged x row two dy tiles.  The plan -- strips, row blocks, the parts of both channel
// axes, the block-id decode with its XCD remap -- is splitconv_wgrad_plan.hpp, which tests/wgrad_plan_check.cpp walks on the CPU.
//
// The global loads of a staged row are unconditional (addresses clamped into the row, zeros selected afterwards; float4 where
// every row starts on a 16-byte boundary), held in registers, and issued one row ahead: they are in flight while the current
// row is multiplied.
//
// Summation order is fixed and the chain is bounded.  Per staged row (at most 64 pixels, 4 MFMA steps) an accumulator starts
// from zero and takes FIRST the five small products of every step -- one x plane at a time, so that only its three shifted
// fragments are live: (a0,b2); (a1,b1) (a0,b1); (a2,b0) (a1,b0), together 2^-8 of the row's sum, so their roundings are
// negligible -- THEN the (a0,b0) products: at most 4 roundings at the row's magnitude.  The row's
// sum is added to the running total with a plain fp32 add (one rounding per row at the chunk's magnitude, at most 128 rows per
// chunk), the chunk's total goes to the workspace, and splitconv_wgrad_finish_kernel adds the chunks in ascending order in
// float64 and rounds once.  No atomics: two calls are bitwise equal.
#include <climits>
#include <cstdint>

#include "splitbf16.hpp"
#include "splitconv_wgrad_plan.hpp"

namespace {
using namespace splitbf16;
using namespace wgrad_plan;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int DY_CS = 3 * G + 1;   // 16-byte slots per dy channel, [plane][group]; odd
constexpr int X_CS = 9 * G + 1;    // 16-byte slots per x channel, [ring row][plane][group]; odd
constexpr int XH_CS = 9 * G + 1;   // dwords per x channel of the neighbour pairs, same order; odd

template <int KT, int CT>
struct Lds {
  static constexpr int DY = 0;
  static constexpr int X = KT * 32 * DY_CS * 16;
  static constexpr int XH = X + CT * 32 * X_CS * 16;
  static constexpr int BYTES = XH + CT * 32 * XH_CS * 4;  // CT = 1: 59 520 / 72 320 for KT = 1 / 2; CT = 2: 106 240 / 119 040
};

__device__ __forceinline__ unsigned bf16_bits(__bf16 b) { return (unsigned)__builtin_bit_cast(unsigned short, b); }

// Eight consecutive floats of a row from column col0 (a multiple of 8): zero where !valid or beyond W.  Every load is
// unconditional and its address clamped into the row -- `row` is a real row of the tensor also where !valid -- so the loads
// of a staging pass are all in flight together and no address outside the tensor is formed.  VEC: W % 4 == 0 and the rows
// 16-byte aligned (host-checked), so two float4 do it.
struct Run {  // a staging item in registers: eight pixels and, for x, the two neighbours
  float4 a, b;
  float l, r;
};
template <bool VEC>
__device__ __forceinline__ void load_run(const float* __restrict__ row, int col0, int W, bool valid, Run& o) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (VEC) {
    const bool in0 = col0 < W, in1 = col0 + 4 < W;
    const float4 t0 = *reinterpret_cast<const float4*>(row + (in0 ? col0 : 0));
    const float4 t1 = *reinterpret_cast<const float4*>(row + (in1 ? col0 + 4 : 0));
    o.a = valid && in0 ? t0 : z;
    o.b = valid && in1 ? t1 : z;
  } else {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = row[min(col0 + e, W - 1)];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (valid && col0 + e < W) ? t[e] : 0.f;
    o.a = make_float4(t[0], t[1], t[2], t[3]);
    o.b = make_float4(t[4], t[5], t[6], t[7]);
  }
}

// grid: decode_block(blockIdx.x): (chunk, output-channel part, input-channel part), the latter fastest, behind the XCD remap:
// the workgroups that share a chunk's dy rows and x tiles run together on one L2.  ws: [chunk][tap][K][C] partial sums.
// Three waves per SIMD where two workgroups of <2, 1> or the twelve waves of one <2, 2> share a CU (float4 loads only).
template <int KT, int CT, bool VEC>
__global__ __launch_bounds__(192 * KT * CT, VEC && KT == 2 ? 3 : 2) void splitconv_wgrad_kernel(
    const float* __restrict__ x, long x_bs, const float* __restrict__ dy, long dy_bs, float* __restrict__ ws, int C, int K, int H,
    int W, const Launch l, int SG, int RPC) {
  constexpr int NT = 192 * KT * CT;
  using L = Lds<KT, CT>;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned* const xh = reinterpret_cast<unsigned*>(lds + L::XH);
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int tile = wv / 3, tr = wv - 3 * tile, ctl = tile / KT, ktl = tile - KT * ctl;
  const Block blk = decode_block(blockIdx.x, gridDim.x, l);
  const int chunk = blk.chunk, strip = blk.strip, n = blk.n, kt0 = blk.kt0, ct0 = blk.ct0;
  // one past the workgroup's last input / output channel: a part may be one tile short of CT / KT
  const int cend = min(C, (ct0 + blk.ctn) * 32), kend = min(K, (kt0 + blk.ktn) * 32);
  const int h0 = blk.rb * RPC, h1 = min(H, h0 + RPC);
  const int GW = (W + 7) >> 3, g0 = strip * SG, gcount = min(SG, GW - g0), nsteps = (gcount + 1) >> 1;
  const long HWl = (long)H * W;
  const float* const xn = x + (long)n * x_bs;
  const float* const dyn = dy + (long)n * dy_bs;

  // Staging items: (x channel, group) for the CT tiles' channels, then (dy channel, group); item j of a thread is number
  // tid + j NT (256 CT x items: whole waves take one kind).  fetch() issues an item's global loads into registers, commit() splits
  // the values and stores the planes: the loads of row h + 1 are in flight while row h is multiplied.
  constexpr int NX = CT * 32 * G, NITEM = NX + KT * 32 * G, NSLOT = (NITEM + NT - 1) / NT;
  Run pf[NSLOT];
  // yx: the x row (any row: outside the image it is zeros); ydy: the dy row, a row of the image, or -1 for none
  const auto fetch = [&](int yx, int ydy) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const int i = tid + j * NT;
      if (i < NX) {
        const int cl = i / G, g = i - cl * G;
        const int c = ct0 * 32 + cl, col0 = (g0 + g) * 8;
        const bool valid = yx >= 0 && yx < H && c < cend && g < gcount;
        const float* row = xn + (valid ? (long)c * HWl + (long)yx * W : 0);
        load_run<VEC>(row, col0, W, valid, pf[j]);
        // the two neighbours: clamped to the row so that the load needs no branch, zero outside it
        const float vl = row[max(col0 - 1, 0)], vr = row[min(col0 + 8, W - 1)];
        pf[j].l = (valid && col0 > 0) ? vl : 0.f;
        pf[j].r = (valid && col0 + 8 < W) ? vr : 0.f;
      } else if (i < NITEM && ydy >= 0) {
        const int kl = (i - NX) / G, g = (i - NX) - kl * G;
        const int k = kt0 * 32 + kl, col0 = (g0 + g) * 8;
        const bool valid = k < kend && g < gcount;
        const float* row = dyn + (valid ? (long)k * HWl + (long)ydy * W : 0);
        load_run<VEC>(row, col0, W, valid, pf[j]);
      }
    }
  };
  const auto commit = [&](int yx, int ydy) __attribute__((always_inline)) {
    const int slot = (yx + 3) % 3;
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const int i = tid + j * NT;
      if (i < NX) {
        const int cl = i / G, g = i - cl * G;
        const float v[8] = {pf[j].a.x, pf[j].a.y, pf[j].a.z, pf[j].a.w, pf[j].b.x, pf[j].b.y, pf[j].b.z, pf[j].b.w};
        bf16x8 o[3];
#pragma unroll
        for (int e = 0; e < 8; ++e) {  // split8's loop in its own text, here and below: through split8 this kernel measured 2 % slower
          const Split s(v[e]);
          o[0][e] = s.p[0], o[1][e] = s.p[1], o[2][e] = s.p[2];
        }
        const Split sl(pf[j].l), sr(pf[j].r);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const int at = (slot * 3 + p) * G + g;
          *reinterpret_cast<bf16x8*>(lds + L::X + (cl * X_CS + at) * 16) = o[p];
          xh[cl * XH_CS + at] = (bf16_bits(sl.p[p]) << 16) | bf16_bits(sr.p[p]);  // pixel 8g - 1 above pixel 8g + 8
        }
      } else if (i < NITEM && ydy >= 0) {
        const int kl = (i - NX) / G, g = (i - NX) - kl * G;
        const float v[8] = {pf[j].a.x, pf[j].a.y, pf[j].a.z, pf[j].a.w, pf[j].b.x, pf[j].b.y, pf[j].b.z, pf[j].b.w};
        bf16x8 o[3];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const Split s(v[e]);
          o[0][e] = s.p[0], o[1][e] = s.p[1], o[2][e] = s.p[2];
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(lds + L::DY + (kl * DY_CS + p * G + g) * 16) = o[p];
      }
    }
  };

  f32x16 tot[3];
  acc_zero(tot);

  const unsigned char* const a_base = lds + L::DY + ((ktl * 32 + r32) * DY_CS + hh) * 16;
  fetch(h0 - 1, -1);
  commit(h0 - 1, -1);
  fetch(h0, -1);
  commit(h0, -1);
  fetch(h0 + 1, h0);
  for (int h = h0; h < h1; ++h) {
    if (h > h0) __syncthreads();  // every wave is done with row h - 1: its dy row and the ring slot of x row h - 2 are free
    commit(h + 1, h);
    __syncthreads();
    fetch(h + 2, h + 1 < h1 ? h + 1 : -1);  // (past the chunk: the x row is loaded for nothing, once)
    const int slot = (h + tr + 2) % 3;  // x row h + tr - 1
    const unsigned char* const b_base = lds + L::X + ((ctl * 32 + r32) * X_CS + slot * 3 * G + hh) * 16;
    const unsigned* const bh_base = xh + (ctl * 32 + r32) * XH_CS + slot * 3 * G + hh;
    if (ctl >= blk.ctn || ktl >= blk.ktn) continue;  // (wave-uniform) a part one tile short: this wave has no tile, it only stages
    f32x16 acc[3];
    acc_zero(acc);
    // the x fragments of plane p for the three tap columns: the aligned run and the two runs shifted by one pixel
    const auto x_frags = [&](int p, int t, bf16x8 (&bs)[3]) __attribute__((always_inline)) {
      const u32x4 d = *reinterpret_cast<const u32x4*>(b_base + (p * G + 2 * t) * 16);
      const unsigned nb = bh_base[p * G + 2 * t];
      const unsigned m1 = __builtin_amdgcn_alignbit(d.y, d.x, 16), m2 = __builtin_amdgcn_alignbit(d.z, d.y, 16),
                     m3 = __builtin_amdgcn_alignbit(d.w, d.z, 16);
      const u32x4 lo = {__builtin_amdgcn_alignbit(d.x, nb, 16), m1, m2, m3};  // pixels 8g - 1 .. 8g + 6: tap column 0
      const u32x4 hi = {m1, m2, m3, __builtin_amdgcn_alignbit(nb, d.w, 16)};  // pixels 8g + 1 .. 8g + 8: tap column 2
      bs[0] = __builtin_bit_cast(bf16x8, lo);
      bs[1] = __builtin_bit_cast(bf16x8, d);
      bs[2] = __builtin_bit_cast(bf16x8, hi);
    };
    // pass 0: the five small products of every step while the accumulator is small, one x plane at a time (its three
    // fragments are all that is live): (a0,b2); (a1,b1) (a0,b1); (a2,b0) (a1,b0) -- (dy plane, x plane)
#pragma unroll 1
    for (int t = 0; t < nsteps; ++t) {  // the lane's group is 2 t + hh
      bf16x8 a[3], bs[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8*>(a_base + (p * G + 2 * t) * 16);
#pragma unroll
      for (int p = 2; p >= 0; --p) {
        x_frags(p, t, bs);
#pragma unroll
        for (int pa = 2 - p; pa >= (p == 0 ? 1 : 0); --pa)
#pragma unroll
          for (int s = 0; s < 3; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa], bs[s], acc[s], 0, 0, 0);
      }
    }
    // pass 1: the (a0, b0) products on top
#pragma unroll 1
    for (int t = 0; t < nsteps; ++t) {
      bf16x8 bs[3];
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(a_base + (2 * t) * 16);
      x_frags(0, t, bs);
#pragma unroll
      for (int s = 0; s < 3; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bs[s], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) tot[s] = tot[s] + acc[s];
  }
  // accumulator register i of lane (r32, hh) is output channel acc_channel(i, hh) of the tile, input channel r32
  const int c = (ct0 + ctl) * 32 + r32;
  if (c < cend) {
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = 32 * (kt0 + ktl) + acc_channel(i, hh);
        if (k < kend) ws[ws_index(chunk, tr * 3 + s, k, c, K, C)] = tot[s][i];
      }
    }
  }
}

// dw[k][c][tap] = the chunks' partial sums added in ascending order in float64
__global__ __launch_bounds__(256) void splitconv_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw, int K,
                                                                       int C, int chunks) {
  const int KC = K * C, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * KC) return;
  const int tap = e / KC, kc = e - tap * KC;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += (double)ws[(long)ch * 9 * KC + e];
  dw[(long)kc * 9 + tap] = (float)s;
}

template <int KT, int CT, bool VEC>
int launch(const float* x, long x_bs, const float* dy, long dy_bs, float* ws, int C, int K, int H, int W, const Launch& l,
           const Plan& p, hipStream_t st) {
  if constexpr (CT > plan_ct(KT, VEC)) {
    return ARFLOW_ESHAPE;  // make_launch never asks for it: not built
  } else {
    using L = Lds<KT, CT>;
    if (const int rc = allow_dynamic_lds<&splitconv_wgrad_kernel<KT, CT, VEC>>(L::BYTES)) return rc;
    if (l.blocks > INT_MAX) return ARFLOW_ESHAPE;
    hipLaunchKernelGGL((splitconv_wgrad_kernel<KT, CT, VEC>), dim3((unsigned)l.blocks), dim3(192 * KT * CT), L::BYTES, st, x, x_bs, dy,
                       dy_bs, ws, C, K, H, W, l, p.SG, p.RPC);
    return af_launch_status();
  }
}
}  // namespace

extern "C" long arflow_splitconv_wgrad_ws_bytes(int N, int C, int K, int H, int W) {
  if (!shape_ok(N, C, K, H, W)) return ARFLOW_ESHAPE;
  const Plan p = make_plan(N, C, K, H, W);
  if (p.chunks > INT_MAX) return ARFLOW_ESHAPE;
  return ws_bytes(p, K, C);
}

extern "C" int arflow_splitconv_wgrad(const float* x, long x_bstride, const float* dy, long dy_bstride, float* dw, void* ws, int N,
                                      int C, int K, int H, int W, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(dy);
  AF_REQUIRE_PTR(dw);
  AF_REQUIRE_PTR(ws);
  AF_REQUIRE(shape_ok(N, C, K, H, W), ARFLOW_ESHAPE);
  AF_REQUIRE(af_stride_ok(x_bstride, N, (long)C * H * W) && af_stride_ok(dy_bstride, N, (long)K * H * W), ARFLOW_ESHAPE);
  AF_REQUIRE(x_bstride >= 0 && dy_bstride >= 0 && x_bstride <= LONG_MAX / N && dy_bstride <= LONG_MAX / N, ARFLOW_ESHAPE);
  AF_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw) & 3) == 0 && af_aligned16(ws), ARFLOW_EPARAM);
  const Plan p = make_plan(N, C, K, H, W);
  AF_REQUIRE(p.chunks <= INT_MAX, ARFLOW_ESHAPE);
  hipStream_t st = (hipStream_t)stream;
  // float4 loads where every row starts on a 16-byte boundary
  const bool vec = W % 4 == 0 && af_vec4_ok(x, x_bstride, N) && af_vec4_ok(dy, dy_bstride, N);
  const Launch l = make_launch(p, vec);  // one launch: the parts of both channel axes are decoded from the block id
  const auto go = [&](auto kt_c, auto ct_c, auto vec_c) {
    return launch<decltype(kt_c)::value, decltype(ct_c)::value, decltype(vec_c)::value>(x, x_bstride, dy, dy_bstride, (float*)ws, C, K, H,
                                                                                        W, l, p, st);
  };
  const auto go_ct = [&](auto kt_c, auto vec_c) {
    return l.ct == 1 ? go(kt_c, std::integral_constant<int, 1>{}, vec_c) : go(kt_c, std::integral_constant<int, 2>{}, vec_c);
  };
  const auto go_kt = [&](auto vec_c) {
    return l.kt == 1 ? go_ct(std::integral_constant<int, 1>{}, vec_c) : go_ct(std::integral_constant<int, 2>{}, vec_c);
  };
  if (const int rc = vec ? go_kt(std::true_type{}) : go_kt(std::false_type{})) return rc;
  hipLaunchKernelGGL(splitconv_wgrad_finish_kernel, dim3((unsigned)af_cdiv((long)9 * K * C, 256)), dim3(256), 0, st,
                     (const float*)ws, dw, K, C, (int)p.chunks);
  return af_launch_status();
}
