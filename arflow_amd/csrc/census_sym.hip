// Pair-symmetric form of the fused census + warp kernels (census_warp.hip) for gfx950.
//
// The soft census distance of utils/uflow_utils.py:241-279 compares, for every pixel p and every offset k of the
// (2R+1)^2 patch, t(p,k) = d / sqrt(0.81 + d^2) with d = grey(p+k) - grey(p), between the two images:
//     ham(p) = sum_k h(p,k),   h = e^2 / (0.1 + e^2),   e = t_a(p,k) - t_b(p,k).
// Seen from the other end of the pair, d(p+k,-k) = -d(p,k), so e flips sign and h(p+k,-k) = h(p,k): every
// UNORDERED pair of pixels needs its two rsq and one rcp ONCE, not twice (the kernels are transcendental/VALU
// bound: 147 transcendentals per pixel in the ordered form).  With K+ = the 24 offsets of the lower half plane
// (ky > 0, or ky = 0 and kx > 0; the centre contributes 0):
//     ham(q) = sum_{k in K+} h(q,k)  +  sum_{k in K+} h(q-k,k)
// -- a pixel evaluates its own 24 "forward" pairs and receives the other 24 from the pixels above / left of it.
// The backward has the same structure: with c = d h / d d_b (odd in d) and w = d loss / d ham,
//     d loss / d grey_b(q) = - sum_{k in K+} (w(q)+w(q+k)) c(q,k) + sum_{k in K+} (w(q-k)+w(q)) c(q-k,k).
//
// Layout.  A workgroup (256 lanes, 4 pixels each) walks DOWN a strip of SW = 56 output columns in chunks of
// CH = 16 rows.  Lanes cover 64 columns (the strip + 4 each side: the senders of the pairs whose receiver is in the
// strip).  Per chunk, for ky = 0..R: every lane evaluates the pairs (p, p+(kx,ky)) of its 4 pixels, keeps them
// for p ("own" role) and writes them as one ds_write_b128 per kx into an LDS plane V[kx][row][col]; after a
// barrier every lane reads the values addressed to ITS pixels from V[kx][row-ky][col-kx] (two aligned
// ds_read_b128 + a compile-time shift).  The rows a chunk needs from the chunk above it (row-ky < 0) come from a
// small carry buffer the previous chunk filled, so only the first chunk of a strip recomputes rows (R of them).
// Pair evaluations per output pixel: 24 * (64/56) * (16n/(16n-R)) ~ 29-31 instead of 48.
//
// The tile of image b is sampled through the flow while it is filled (see census_warp.hip), the mask is evaluated
// per pixel, the backward ends in d loss / d flow.  Every plane access is linear across the wave (16 lanes x 16 B
// per row, rows contiguous): conflict-free.
#include "census_tile.hpp"
#include "taps.hpp"

namespace {
namespace census_sym {
using census4::f32x4;
using census4::read12;
constexpr int NT = 256, SW = 56, LW = 64, CH = 16, PITCH = 128, MAXR = 3;
constexpr int TROWS = CH + MAXR;          // tile rows per chunk (senders + their lower neighbours)
constexpr int VPLANE = CH * LW;           // one kx plane of V
constexpr int GUARD = 4;                  // floats before / after V and the carry (non-output lanes read 1 float4 outside)

__host__ __device__ constexpr int carry_base(int ky) { return (2 * MAXR + 1) * LW * (ky * (ky - 1) / 2); }  // rows before ky
constexpr int CARRY = carry_base(MAXR + 1);  // floats per parity

// warped grey tile: rows [cy0, cy0+CH+R), tile columns 1 .. 70 (image tx0+1 ..); zero outside the image.
// Rounds of UNR pixels per thread: all flow loads of a round in flight together, then all 4 x UNR taps.
template <int R>
__device__ __forceinline__ void load_warped(float* __restrict__ tile, const float* __restrict__ gsrc,
                                            const float* __restrict__ flow, int H, int W, int cy0, int tx0, int tid) {
  constexpr int NR = CH + R, NC = 70, UNR = 3;
  const long cs = (long)H * W;
#pragma unroll 1
  for (int i0 = tid; i0 < NR * NC; i0 += NT * UNR) {
    float u[UNR], v[UNR];
    int gx[UNR], gy[UNR], dst[UNR];
    bool in[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int i = i0 + k * NT;
      const int r = i / NC, c = i - r * NC;
      gy[k] = cy0 + r;
      gx[k] = tx0 + 1 + c;
      dst[k] = i < NR * NC ? r * PITCH + 1 + c : -1;
      in[k] = dst[k] >= 0 && gy[k] >= 0 && gy[k] < H && gx[k] >= 0 && gx[k] < W;
      const long o = in[k] ? (long)gy[k] * W + gx[k] : 0;
      u[k] = flow[o];
      v[k] = flow[o + cs];
    }
    float a[UNR][4];
    TapPlan p[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const Taps t = make_taps((float)gx[k], (float)gy[k], u[k], v[k], H, W, H, W, ARFLOW_PAD_ZEROS, true, ARFLOW_NORM_UFLOW);
      p[k] = plan_taps(t, H, W);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[k][q] = gsrc[p[k].o[q]];
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k)
      if (dst[k] >= 0) tile[dst[k]] = in[k] ? tap_blend(p[k], a[k]) : 0.f;
  }
}

__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  f32x4 t = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p) = t;
}
// the 4 values addressed to this lane's pixels from a plane row: columns 4g-kx .. 4g-kx+3 (kx is a compile-time
// constant after unrolling: the indices below fold)
__device__ __forceinline__ void ld_shift(const float* rowbase /* column 4g of the source row */, int kx, float (&o)[4]) {
  if (kx == 0) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(rowbase);
    o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
  } else {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(rowbase + (kx > 0 ? -4 : 0));
    const f32x4 hi = *reinterpret_cast<const f32x4*>(rowbase + (kx > 0 ? 0 : 4));
    const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int S = kx > 0 ? 4 - kx : -kx;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = w[S + j];
  }
}

struct Lds {
  float* ga;
  float* gb;
  float* gw;  // backward only
  float* V;
  float* carry;  // [2][CARRY]
};

// One ky pass, sender side: evaluate the pairs (p, p + (kx, KY)) of this lane's 4 pixels, accumulate the own
// role, publish the values for the other end of each pair.
template <int R, int KY, bool BWD>
__device__ __forceinline__ void pass_send(const Lds& L, int g, int ly, int parity, const float (&ca)[4], const float (&cb)[4],
                                          const float (&cg)[4], float (&acc)[4]) {
  float wa[12], wb[12], wg[12];
  // the window offset is laundered: without it hipcc hoists the window reads of all four passes above the first
  // barrier (they do not alias V) and keeps ~60 VGPRs per pass alive -- 256 + spills for R = 3
  int woff = (ly + KY) * PITCH + 4 * g;
  asm volatile("" : "+v"(woff));
  read12(L.ga + woff, wa);
  read12(L.gb + woff, wb);
  if (BWD) read12(L.gw + woff, wg);
#pragma unroll
  for (int kx = -R; kx <= R; ++kx) {
    if (KY == 0 && kx <= 0) continue;
    const int kxi = KY == 0 ? kx - 1 : kx + R;
    float v[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int k = 4 + p + kx;  // window column of the neighbour
      if (!BWD) {
        v[p] = pair_dist(ca[p], cb[p], wa[k], wb[k]);
        acc[p] += v[p];
      } else {
        v[p] = (wg[k] + cg[p]) * pair_grad(wa[k], wb[k], ca[p], cb[p]);  // (the derivative at the NEIGHBOUR: odd)
        acc[p] -= v[p];
      }
    }
    st4(L.V + (kxi * CH + ly) * LW + 4 * g, v);
    if (KY > 0 && ly >= CH - KY)
      st4(L.carry + parity * CARRY + carry_base(KY) + (kxi * KY + (ly - (CH - KY))) * LW + 4 * g, v);
    // two kx (8 independent pixel chains) at a time: left alone the scheduler interleaves all 28 chains of a pass
    // and needs > 256 VGPRs
    if ((kx & 1) == 0) __builtin_amdgcn_sched_barrier(0);
  }
}

// receiver side: the sum of the values of the pairs (q - (kx, KY), q) for this lane's 4 pixels
struct F4 {
  float v[4];
};
template <int R, int KY>
__device__ __forceinline__ F4 pass_recv(const float* base /* column 4g of the source row, plane 0 */, int plane) {
  F4 s = {{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int kx = -R; kx <= R; ++kx) {
    if (KY == 0 && kx <= 0) continue;
    const int kxi = KY == 0 ? kx - 1 : kx + R;
    float r[4];
    ld_shift(base + kxi * plane, kx, r);
#pragma unroll
    for (int p = 0; p < 4; ++p) s.v[p] += r[p];
  }
  return s;
}

template <int R, int KY, bool BWD>
__device__ __forceinline__ void all_passes(const Lds& L, int g, int ly, int parity, const float (&ca)[4], const float (&cb)[4],
                                           const float (&cg)[4], float (&acc)[4]) {
  pass_send<R, KY, BWD>(L, g, ly, parity, ca, cb, cg, acc);
#ifndef SYM_AB_NO_BARRIER  // A/B timing only: racing exchange -> wrong results
  __syncthreads();
#endif
  {
    const bool from_carry = ly < KY;
    const float* base = from_carry ? L.carry + (parity ^ 1) * CARRY + carry_base(KY) + ly * LW + 4 * g
                                   : L.V + (ly - KY) * LW + 4 * g;
    const F4 r = pass_recv<R, KY>(base, from_carry ? KY * LW : VPLANE);
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] += r.v[p];
  }
#ifndef SYM_AB_NO_BARRIER
  __syncthreads();  // V is rewritten by the next pass / the tiles by the next chunk
#endif
  if constexpr (KY < R) all_passes<R, KY + 1, BWD>(L, g, ly, parity, ca, cb, cg, acc);
}

// strip s of an image: output rows [sy0, sy1), output columns [sx0, sx0+SW)
template <int R, bool BWD>
__global__ __launch_bounds__(NT, 2) void kernel(const float* __restrict__ gray_a, const float* __restrict__ gray_b,
                                            const float* __restrict__ flow, long fbs,
                                            const float* __restrict__ occ_small,  // fwd
                                            float* __restrict__ mask_out,         // fwd
                                            float* __restrict__ dham,             // fwd: out, bwd: in
                                            float* __restrict__ sums, int nrows,  // fwd
                                            const float* __restrict__ scale,      // bwd
                                            float* __restrict__ gflow,            // bwd
                                            int nimg, int H, int W, int strip_h) {
  __shared__ __attribute__((aligned(16))) float lds_ga[TROWS * PITCH];
  __shared__ __attribute__((aligned(16))) float lds_gb[TROWS * PITCH];
  __shared__ __attribute__((aligned(16))) float lds_gw[BWD ? TROWS * PITCH : 4];
  __shared__ __attribute__((aligned(16))) float lds_v[GUARD + (2 * MAXR + 1) * VPLANE + GUARD];
  __shared__ __attribute__((aligned(16))) float lds_c[GUARD + 2 * CARRY + GUARD];
  __shared__ float red[2 * (NT / 64)];
  const int nsx = (W + SW - 1) / SW, nsy = (H + strip_h - 1) / strip_h;
  int stx, sty, b;
  if (!af_tile_of_block(nsx, nsy, nimg, stx, sty, b)) {
    if (!BWD && threadIdx.x == 0) af_store_partial(sums, nrows, 0.f, 0.f, 0.f);  // padding workgroup: its row must be defined
    return;
  }
  const int sx0 = stx * SW, sy0 = sty * strip_h, sy1 = min(sy0 + strip_h, H);
  const long cs = (long)H * W;
  const float* fl = flow + b * fbs;
  const float* ga_p = gray_a + b * cs;
  const float* gb_p = gray_b + b * cs;
  Lds L;
  L.ga = lds_ga, L.gb = lds_gb, L.gw = lds_gw, L.V = lds_v + GUARD, L.carry = lds_c + GUARD;
  const float* occ = (!BWD && occ_small) ? occ_small + (long)b * (H / 4) * (W / 4) : nullptr;
  float part[2] = {0.f, 0.f};
  // tile columns 1 and 70 .. 71 margins of gb are never written by the sampler: zero them once
  for (int i = threadIdx.x; i < TROWS * 2; i += NT) lds_gb[(i >> 1) * PITCH + ((i & 1) ? 71 : 0)] = 0.f;
  int parity = 0;
  for (int cy0 = sy0 - R; cy0 < sy1; cy0 += CH, parity ^= 1) {
    // the lane index is laundered once per chunk: otherwise LICM hoists every lane-dependent address, mask weight
    // and predicate of the ~5000-instruction body out of this loop and keeps > 256 of them alive (spills)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int g = tid & 15, ly = tid >> 4;
    const int x0 = sx0 - 4 + 4 * g;  // image column of this lane's first pixel
    const bool out_col = g >= 1 && g <= SW / 4 && x0 < W;
#ifdef SYM_AB_NO_WARP  // A/B timing only (tools/): plain tile instead of the sampled one -> wrong results
    census4::load_plane_rows<CH + R>(lds_gb, gb_p, H, W, cy0, sx0 - 8, tid);
#else
    load_warped<R>(lds_gb, gb_p, fl, H, W, cy0, sx0 - 8, tid);
#endif
    census4::load_plane_rows<CH + R>(lds_ga, ga_p, H, W, cy0, sx0 - 8, tid);
    if (BWD) census4::load_plane_rows<CH + R>(lds_gw, dham + b * cs, H, W, cy0, sx0 - 8, tid);
    __syncthreads();
    const int y = cy0 + ly;
    const bool out = out_col && y >= sy0 && y < sy1;  // this lane's 4 pixels are outputs of this strip
    // backward: the corner differences of the grey plane at this lane's pixels (gathers in flight during the passes)
    float cdx[4] = {0.f, 0.f, 0.f, 0.f}, cdy[4] = {0.f, 0.f, 0.f, 0.f};
    if (BWD && out) corner_grads4(gb_p, fl, x0, y, H, W, cdx, cdy);
    float ca[4], cb[4], cg[4] = {0.f, 0.f, 0.f, 0.f}, acc[4] = {0.f, 0.f, 0.f, 0.f};
    {
      float w0[12];
      read12(lds_ga + ly * PITCH + 4 * g, w0);
#pragma unroll
      for (int p = 0; p < 4; ++p) ca[p] = w0[4 + p];
      read12(lds_gb + ly * PITCH + 4 * g, w0);
#pragma unroll
      for (int p = 0; p < 4; ++p) cb[p] = w0[4 + p];
      if (BWD) {
        read12(lds_gw + ly * PITCH + 4 * g, w0);
#pragma unroll
        for (int p = 0; p < 4; ++p) cg[p] = w0[4 + p];
      }
    }
    all_passes<R, 0, BWD>(L, g, ly, parity, ca, cb, cg, acc);
    if (out) {
      const long o = (long)y * W + x0;
      if (!BWD) {
        float mv[4], dh[4];
        masked_loss4(fl, occ, acc, x0, y, H, W, R, mv, dh, part);
        if (mask_out) store_row<4>(mask_out + (long)b * cs + o, mv);
        store_row<4>(dham + (long)b * cs + o, dh);
      } else {
        store_flow_grad<4>(gflow + (long)b * 2 * cs + o, cs, dir_scale(scale, 0, b), acc, cdx, cdy);
      }
    }
  }
  if (!BWD) {
    af_block_sum<2>(part, red);
    if (threadIdx.x == 0) af_store_partial(sums, nrows, part[0], part[1], 0.f);
  }
}

}  // namespace census_sym
}  // namespace

// strip height: 16 n - R rows (n chunks, the first one recomputes R rows of its upper neighbour), n chosen so that
// the launch has at least ~3 workgroups per CU
static int census_sym_strip_h(int B, int H, int W, int R) {
  const long per_row_band = (long)B * af_cdiv(W, census_sym::SW);
  int n = 4;
  while (n > 1 && per_row_band * af_cdiv(H, 16 * n - R) < 3 * 256) --n;
  return 16 * n - R;
}

static unsigned census_sym_grid(int B, int H, int W, int strip_h) {
  return af_grid_for_tiles((long)af_cdiv(W, census_sym::SW) * af_cdiv(H, strip_h) * B);
}

int census_sym_fwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* occ_small,
                   float* mask_out, float* dham, float* sums, int nrows, int B, int H, int W, int radius, hipStream_t st) {
  namespace cs = census_sym;
  const int sh = census_sym_strip_h(B, H, W, radius);
  dim3 g(census_sym_grid(B, H, W, sh));
  af_dispatch_radius(radius, [&](auto R) {
    hipLaunchKernelGGL((cs::kernel<decltype(R)::value, false>), g, dim3(cs::NT), 0, st, gray_a, gray_b, flow, fbs, occ_small,
                       mask_out, dham, sums, nrows, nullptr, nullptr, B, H, W, sh);
  });
  return af_launch_status();
}

int census_sym_bwd(const float* gray_a, const float* gray_b, const float* flow, long fbs, const float* dham,
                   const float* scale, float* gflow, int B, int H, int W, int radius, hipStream_t st) {
  namespace cs = census_sym;
  const int sh = census_sym_strip_h(B, H, W, radius);
  dim3 g(census_sym_grid(B, H, W, sh));
  float* dh = const_cast<float*>(dham);
  af_dispatch_radius(radius, [&](auto R) {
    hipLaunchKernelGGL((cs::kernel<decltype(R)::value, true>), g, dim3(cs::NT), 0, st, gray_a, gray_b, flow, fbs, nullptr, nullptr,
                       dh, nullptr, 0, scale, gflow, B, H, W, sh);
  });
  return af_launch_status();
}
