// Deterministic bilinear scatter: the fixed-order form of the two 4-tap scatters of the hot path --
//   WARP : d loss / d src of the bilinear warp, gsrc[b,c,q] = sum over (target pixel p, tap k) landing on q of w_k(p) gout[b,c,p]
//          (lds_scatter::warp_bwd_src_kernel and its fallbacks, warp.hip: float atomics);
//   SPLAT: the forward splat of compute_range_map / get_corresponding_map, out[b,q] = sum of w_k(p)
//          (splat_kernel, warp.hip: 2^-22 fixed point in LDS + one float atomic per cell and tile)
// -- selected by the launchers while deterministic mode is on (arflow_set_deterministic).  The taps are the default
// kernels' own (make_taps / plan_taps and splat_taps, taps.hpp), so the SET of terms of every output element is identical;
// only the order they are added in is pinned.
//
// Owner computes.  One workgroup OWNS an 8 x 32 tile of output cells, one cell per thread, and walks every target pixel of
// the sample in ascending index, 256 at a time:
//   1. each thread computes the four taps of its pixel p and keeps those that land in the tile;
//   2. the kept (p, k) pairs are compacted into an LDS list IN ORDER (p ascending, then k) -- a wave prefix sum over
//      the per-thread counts plus the four wave totals, no atomics of any kind;
//   3. every thread walks the list front to back and adds the entries of its own cell: acc = fmaf(w, gout[c, p], acc).
// So the value of a cell is its terms added in ascending (p, k) order, whatever the flow does: a function of the data
// indices alone -- not of workgroup or wave scheduling, atomic arrival or addresses.  Nothing is lost or counted twice when
// every pixel lands on one cell (the list holds all 4 x 256 pairs of a round) or when no tap is inside the image (the
// cells are written as 0); every output element is written by its owner, so there is no zero-fill and no dependence on
// the buffer's previous contents; no scratch memory.
//
// Cost: every tile reads the whole flow of its sample (tiles x H W tap evaluations per sample instead of H W), which at
// the sizes these scatters run at (feature maps and quarter-resolution flows, <= 96 x 160 in the shipped configurations)
// is ~1e6 tap evaluations per sample.  The price of the mode is stated in DESIGN.md section 14, not hidden.
#include "common.hpp"
#include "taps.hpp"

namespace {
namespace det {
constexpr int TX = 32, TY = 8, NT = TX * TY;
static_assert(NT == 256, "a list entry packs the cell (8 bits) and the pixel's slot in the round (8 bits)");

struct Args {
  const float* flow;  // [B,2,H,W], batch stride fbs
  long fbs;
  const float* val;   // WARP: gout [B,C,H,W]
  float* out;         // WARP: gsrc [B,C,Hs,Ws]; SPLAT: [B,1,H,W] (Hs = H, Ws = W)
  int nimg, C, Hs, Ws, H, W;
  int pad, align, norm;  // WARP
  int variant;           // SPLAT (ARFLOW_COORDS_ABS may be set)
};

// the taps of target pixel (px, py): cell coordinates, weight, "lands inside the output"
struct Hit {
  int x[4], y[4];
  float w[4];
  bool ok[4];
};
template <bool SPLAT>
__device__ __forceinline__ Hit taps_of(const Args& a, int px, int py, float u, float v) {
  Hit h;
  if (SPLAT) {
    const bool abs_in = (a.variant & ARFLOW_COORDS_ABS) != 0;
    const SplatTaps t = splat_taps(abs_in ? u : (float)px + u, abs_in ? v : (float)py + v, a.H, a.W, a.variant);
#pragma unroll
    for (int k = 0; k < 4; ++k) h.x[k] = t.xi[k], h.y[k] = t.yi[k], h.w[k] = t.w[k], h.ok[k] = t.ok[k];
  } else {
    const Taps t = make_taps((float)px, (float)py, u, v, a.H, a.W, a.Hs, a.Ws, a.pad, a.align != 0, a.norm);
    const TapPlan p = plan_taps(t, a.Hs, a.Ws);
#pragma unroll
    for (int k = 0; k < 4; ++k) h.x[k] = t.x0 + (k & 1), h.y[k] = t.y0 + (k >> 1), h.w[k] = p.w[k], h.ok[k] = p.ok[k];
  }
  return h;
}

// grid: (af_grid_for_tiles(tiles of the OUTPUT), ceil(C / CCH)); CCH channels per workgroup, one accumulator register
// each.  The flow walk and the list are rebuilt per channel group, and that is the cheaper side: what bounds the kernel is
// the dependent gout reads of the list walk, which want many workgroups in flight.  Measured in the level backward at
// B16 C32 (whole call, rough flows of the random-init network): CCH = 4 -> 1.59 ms at 96 x 160, 0.52 ms at 48 x 80,
// 0.22 ms at 24 x 40; CCH = 32 (one list per tile) -> 3.19 / 1.97 / 1.13 ms.  The launcher uses 4.
template <bool SPLAT, int CCH>
__global__ __launch_bounds__(NT) void scatter_kernel(const Args a) {
  __shared__ int e_key[2][4 * NT];   // (slot of p in the round) << 8 | cell
  __shared__ float e_w[2][4 * NT];
  __shared__ int wave_tot[2][NT / 64];
  int btx, bty, b;
  if (!af_tile_of_block((a.Ws + TX - 1) / TX, (a.Hs + TY - 1) / TY, a.nimg, btx, bty, b)) return;  // whole workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = btx * TX, y0 = bty * TY;
  const int cx = x0 + (tid & 31), cy = y0 + (tid >> 5);  // the cell this thread owns: cell id == tid
  const int c0 = blockIdx.y * CCH;
  const long os = (long)a.H * a.W;
  const float* fb = a.flow + (long)b * a.fbs;
  const float* gp = SPLAT ? nullptr : a.val + ((long)b * a.C + c0) * os;
  float acc[CCH];
#pragma unroll
  for (int c = 0; c < CCH; ++c) acc[c] = 0.f;

  float u = 0.f, v = 0.f;
  if (tid < os) u = fb[tid], v = fb[os + tid];
  const long nround = (os + NT - 1) / NT;
  for (long r = 0; r < nround; ++r) {
    const int buf = (int)(r & 1);
    const long p0 = r * NT, p = p0 + tid;
    float un = 0.f, vn = 0.f;  // the next round's flow is in flight during this one
    if (p + NT < os) un = fb[p + NT], vn = fb[os + p + NT];
    int key[4];
    float w[4];
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) key[k] = 0, w[k] = 0.f;
    if (p < os) {
      const int py = (int)(p / a.W), px = (int)(p - (long)py * a.W);
      const Hit h = taps_of<SPLAT>(a, px, py, u, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int dx = h.x[k] - x0, dy = h.y[k] - y0;
        if (h.ok[k] && (unsigned)dx < (unsigned)TX && (unsigned)dy < (unsigned)TY) {
          m |= 1u << k;
          key[k] = (tid << 8) | (dy * TX + dx);
          w[k] = h.w[k];
        }
      }
    }
    // position of this thread's first entry: pairs of lower threads come first (p ascending)
    const int n = __popc(m);
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wave_tot[buf][wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) {
      const int t = wave_tot[buf][q];
      base += q < wave ? t : 0;
      total += t;
    }
    if (total) {  // workgroup-uniform
      int pos = base + incl - n;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((m >> k) & 1u) e_key[buf][pos] = key[k], e_w[buf][pos] = w[k], ++pos;  // then k ascending
      __syncthreads();
      for (int e = 0; e < total; ++e) {  // every thread reads the same entry: an LDS broadcast
        const int kk = e_key[buf][e];
        if ((kk & 0xff) != tid) continue;
        const float ww = e_w[buf][e];
        if (SPLAT) {
          acc[0] += ww;
        } else {
          const float* g = gp + p0 + (kk >> 8);
#pragma unroll
          for (int c = 0; c < CCH; ++c)
            if (c0 + c < a.C) acc[c] = fmaf(ww, g[(long)c * os], acc[c]);
        }
      }
    }
    // (both LDS buffers alternate: a round's list and totals are rewritten two rounds later, behind the barrier of the
    // round in between, which no thread passes before every thread has finished reading them)
    u = un, v = vn;
  }
  if (cx < a.Ws && cy < a.Hs) {
    const long ss = (long)a.Hs * a.Ws;
    float* o = a.out + ((long)b * a.C + c0) * ss + (long)cy * a.Ws + cx;
#pragma unroll
    for (int c = 0; c < CCH; ++c)
      if (c0 + c < a.C) o[(long)c * ss] = acc[c];
  }
}
}  // namespace det
}  // namespace

// d loss / d src of the warp, fixed order.  Arguments as validated by the warp entry points (warp_check_args, warp.hip).
int af_det_warp_src_launch(const float* gout, const float* flow, float* gsrc, int B, int C, int Hs, int Ws, int H, int W,
                           long flow_bstride, int pad_mode, int align_corners, int norm_mode, hipStream_t st) {
  const det::Args a{flow, flow_bstride, gout, gsrc, B, C, Hs, Ws, H, W, pad_mode, align_corners, norm_mode, 0};
  const long tiles = (long)af_cdiv(Ws, det::TX) * af_cdiv(Hs, det::TY) * B;
  constexpr int CCH = 4;
  const int groups = af_cdiv(C, CCH);
  AF_REQUIRE(groups <= 65535, ARFLOW_ESHAPE);
  hipLaunchKernelGGL((det::scatter_kernel<false, CCH>), dim3(af_grid_for_tiles(tiles), groups), dim3(det::NT), 0, st, a);
  return af_launch_status();
}

// forward splat (variant as arflow_splat_map, ARFLOW_COORDS_ABS included), fixed order; every cell of out written
int af_det_splat_launch(const float* flow, float* out, int B, int H, int W, long flow_bstride, int variant, hipStream_t st) {
  const det::Args a{flow, flow_bstride, nullptr, out, B, 1, H, W, H, W, 0, 0, 0, variant};
  const long tiles = (long)af_cdiv(W, det::TX) * af_cdiv(H, det::TY) * B;
  hipLaunchKernelGGL((det::scatter_kernel<true, 1>), dim3(af_grid_for_tiles(tiles), 1), dim3(det::NT), 0, st, a);
  return af_launch_status();
}
