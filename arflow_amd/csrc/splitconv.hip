// 3x3 convolution (stride 1, zero padding 1, dilation 1) of the WIDE layers on the bf16 matrix cores at fp32 accuracy, for
// gfx950: the dense flow estimators' 147..563 -> 128..32 layers and the context network's 597 -> 128, forward and -- with
// the roles of the channel axes swapped and the taps flipped by the packer -- data gradient.
//
// Arithmetic.  An fp32 number splits EXACTLY into three bf16 numbers, b0 + b1 + b2 == x bit for bit (splitbf16.hpp: Split).
// A product x * w is then nine bf16 products, each exact in the MFMA's fp32 accumulator; the three smallest (b1 w2, b2 w1,
// b2 w2) are below 2^-24 of the product and dropped, the other six are accumulated: (w2,x0) (w1,x1) (w0,x2) (w1,x0) (w0,x1) (w0,x0).
// Six v_mfma_f32_32x32x16_bf16 per 32x32x16 block of fp32-accurate products: 1/6 of the bf16 rate, 2.7x the fp32 MFMA's.
//
// GEMM view: D[k][pixel] = sum over (tap, c) of A[k][(tap, c)] * B[(tap, c)][pixel].  A = weights, packed once per call by
// arflow_splitconv_pack into the three bf16 planes IN FRAGMENT ORDER (a wave's A fragment is 1 KiB contiguous, read straight
// from L2); B = the input: per block of 32 input channels a workgroup loads its halo tile from NCHW, splits every value in
// registers and stores the planes to LDS as [pixel][plane][channel], so that a lane's B fragment (8 consecutive channels of
// one pixel) is one ds_read_b128 and a tap is a pixel offset, not a re-load.  The pixel stride is 3 * 64 + 16 bytes = 13
// 16-byte slots: odd, so the 16 lanes ds_read_b128 serves together fall on 16 different slots of the 256-byte bank row.
//
// A workgroup of 4 waves owns 8 pixel tiles (32 pixels each: PW columns x 32 / PW rows, stacked vertically) and KT <= 2
// tiles of 32 output channels.  A wave holds ONE channel tile x 2 KT pixel tiles -- at KT = 1 two of the eight pixel tiles,
// at KT = 2 four of them for one of the two channel tiles (a weight fragment is then fetched by two
// waves of the workgroup instead of four, a pixel fragment by two instead of one, and LDS has the bandwidth to spare) --
// twice: the accumulators of the current block and the running totals, up to 128 registers.  Two workgroups share a CU
// (2 x 70 KB of LDS, 256 registers per lane): one stages its next block while the other multiplies.  More than 64 output
// channels go over gridDim.y in chunks of equal size (+-1 tile: no tile of zeros is multiplied).
//
// Operand fetch is software-pipelined (DESIGN.md sections 32, 40): the weight fragments of a unit -- one (tap, step) in
// pass 0, three of them in pass 1 -- are requested while the unit before it multiplies, into the second of two register
// buffers of three fragments; the pixel fragments come a unit ahead as well, in halves of two pixel tiles x three planes,
// into a ring of KT + 1 buffers of six fragments (24 + 72 registers at KT = 2: 242..251 in all), through both passes and
// across the block boundary; the staging loads of three items go out together.  Which products are formed, and in which
// order, is untouched.
//
// Summation order is fixed.  Within a block of 32 input channels one MFMA accumulator chain starts from zero and takes, over
// taps row-major and 16-channel steps ascending, FIRST the five small products of every step -- (w2,x0) (w1,x1) (w0,x2)
// (w1,x0) (w0,x1), together 2^-8 of the block's sum, so that their 90 roundings are negligible -- and THEN the 18 (w0,x0)
// products; the blocks' sums are added to the running total in ascending order with plain fp32 adds.  (An MFMA rounds at
// the accumulator's magnitude whatever it adds: one chain over all blocks with the six products interleaved has six full
// roundings per 16 terms where an fp32 kernel has one.  Emulated at 597 x 9 all-positive terms: 27 u of sum |a b| for
// that, 13 u for fp32 partial sums of 16, 4.7 u with the per-block restart, and with the small products first as well
// the figure in tests/test_splitconv_cpu.py.)  No atomics, no split of the reduction: two calls are bitwise equal, in
// every mode.
//
// Batch strides of x and y are arguments (planes, rows and columns dense): a channel slice of a larger tensor is read, and a
// channel slot of one written, in place.  The store can apply bias + LeakyReLU (a runtime branch; the loop above it is the
// same code).  The dense flow estimator runs its five layers that way inside the one tensor x6:
// layer k reads x6[:, off:] and writes x6[:, off - K:off]; no element is both read and written, which __restrict__ needs.
#include <climits>
#include <cstdint>

#include "splitbf16.hpp"

namespace {
using namespace splitbf16;

constexpr int NT = 256;                       // 4 waves
constexpr int CB = 32;                        // input channels per LDS block (two MFMA k-steps)
constexpr int PLANE_BYTES = CB * 2;           // one pixel's channels of one plane
constexpr int PIX_BYTES = 3 * PLANE_BYTES + 16;  // 208: see the header
constexpr int FRAG = 64 * 8;                  // bf16 per wave fragment (32 rows x 16 k)

template <int PW>
struct Geo {
  static constexpr int PR = 32 / PW;    // rows of a pixel tile
  static constexpr int TH = 8 * PR;     // rows of the workgroup's tile
  static constexpr int HW = PW + 2;     // halo tile
  static constexpr int HH = TH + 2;
  static constexpr int NPIX = HH * HW;  // 340 / 324 / 340 for PW = 32 / 16 / 8
  static constexpr int LDS_BYTES = NPIX * PIX_BYTES;
};

// packed: [plane 3][tap 9][nkt = ceil(K / 32)][ncs = 2 ceil(C / 32)][lane 64][8], element j of lane (r = lane & 31, h = lane >> 5)
// = plane of W[k = 32 kt + r][c = 16 cs + 8 h + j][tap], zero where k >= K or c >= C.  transpose_flip: W = w'[c][k][8 - tap].
__global__ __launch_bounds__(NT) void splitconv_pack_kernel(const float* __restrict__ w, bf16x8* __restrict__ packed, int wK, int wC,
                                                            int Kout, int Cin, int nkt, int ncs, int transpose_flip) {
  const int nfrag = 9 * nkt * ncs * 64;
  const int f = blockIdx.x * NT + threadIdx.x;
  if (f >= nfrag) return;
  const int lane = f & 63, cs = (f >> 6) % ncs, kt = ((f >> 6) / ncs) % nkt, tap = (f >> 6) / (ncs * nkt);
  const int k = 32 * kt + (lane & 31), c0 = 16 * cs + 8 * (lane >> 5);
  const auto weight = [&](int j) {
    const int c = c0 + j;
    float v = 0.f;
    if (k < Kout && c < Cin) v = transpose_flip ? w[((long)c * wC + k) * 9 + (8 - tap)] : w[((long)k * wC + c) * 9 + tap];
    return v;
  };
  bf16x8 o[3];
  split8(weight, o);
#pragma unroll
  for (int p = 0; p < 3; ++p) packed[(long)p * nfrag + f] = o[p];
}

template <int KT, int PW>
__global__ __launch_bounds__(NT, 2) void splitconv_kernel(const float* __restrict__ x, long x_bs, const bf16x8* __restrict__ packed,
                                                          float* __restrict__ y, long y_bs, const float* __restrict__ bias, int act,
                                                          float slope, int C, int K, int H, int W, int nkt, int ncs, int kt_first,
                                                          int tiles_x, int tiles_y) {
  using G = Geo<PW>;
  extern __shared__ __align__(16) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int t = blockIdx.x;
  const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, n = t / (tiles_x * tiles_y);
  const int h0 = ty * G::TH, w0 = tx * PW;
  // The wave's tile: ONE channel tile x PT pixel tiles.  KT = 1: the four waves take two pixel tiles each.  KT = 2: waves
  // 0, 1 take the workgroup's first channel tile and waves 2, 3 its second, pixel tiles 0..3 (waves 0, 2) or 4..7 (waves
  // 1, 3) -- a weight fragment is fetched by two waves of the workgroup, not by all four.
  constexpr int PT = 2 * KT;
  constexpr int NH = KT;      // half-units (two pixel tiles each) of a pass-0 unit
  constexpr int NB = KT + 1;  // pixel-fragment buffers: a ring, one unit ahead
  const int ktw = kt_first + blockIdx.y * KT + (KT == 2 ? wv >> 1 : 0);
  const int pt0 = KT == 2 ? 4 * (wv & 1) : 2 * wv;
  const long plane_frags = (long)9 * nkt * ncs * 64;  // fragments (of 8 bf16) per plane

  f32x16 tot[PT];  // running totals; every block of 32 input channels is summed in fresh accumulators first
  acc_zero(tot);

  // the lane's pixel in the first of the wave's pixel tiles: halo-tile byte offset of tap (0, 0), plus its k half
  // (tile pt: pbase + pt * PT_BYTES, a constant apart, so that every LDS address is this one register plus a uniform offset)
  constexpr int PT_BYTES = G::PR * G::HW * PIX_BYTES;
  const int pcol = r % PW, prow0 = pt0 * G::PR + r / PW;
  const int pbase = (prow0 * G::HW + pcol) * PIX_BYTES + hh * 16;
  const float* xn = x + (long)n * x_bs;  // the sample's planes are dense; the batch stride is the caller's
  const long HWl = (long)H * W;
  const unsigned HWu = (unsigned)(H * W);

  // Weight fragments travel one unit ahead of the MFMAs that take them: two register buffers of three
  // fragments; while a unit multiplies out of one, the next unit's loads fill the other, and the wait before
  // the MFMAs retires the older loads only.  The chain runs through both passes and from block to block: the first unit of a
  // block does not depend on LDS and is in flight across the barriers and the staging.  The loads stand between two
  // scheduling barriers that only plain ALU work may cross, so the compiler neither sinks them to their use
  // nor hoists later ones until registers spill.  An address is a wave-uniform pointer (the fragment: scalar arithmetic)
  // plus the lane's 32-bit byte offset wl: no vector add per load.
  constexpr int SCHED_FREE = 0x2 | 0x4;  // VALU, SALU
  const long tap_frags = (long)nkt * ncs * 64;  // fragments from a tap to the next
  // (wl is re-defined by an empty asm at the head of every trip: were its zero-extension hoisted out of the loads' basic
  // block, instruction selection would not see it and the add would be 64-bit VALU again)
  unsigned wl = lane * (unsigned)sizeof(bf16x8);
  const auto pin_wl = [&]() __attribute__((always_inline)) { asm volatile("" : "+v"(wl)); };
  bf16x8 wq[2][3];
  const auto wload = [&](bf16x8 (&d)[3], const bf16x8* base, long o0, long o1, long o2) __attribute__((always_inline)) {
    const auto frag = [&](long o) { return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(base + o) + wl); };
    d[0] = frag(o0), d[1] = frag(o1), d[2] = frag(o2);
  };
  const bf16x8* wblk = packed + (long)ktw * ncs * 64;  // the block's (tap 0, tile ktw, step 0) fragment of plane 0: lane 0's
  wload(wq[0], wblk, 0, plane_frags, 2 * plane_frags);
  // The pixel fragments likewise, out of LDS: byte offsets from the lane's pixel of tap (0, 0).  A buffer holds two pixel
  // tiles x three fragments (slot 3 ptl + i): half s of a unit is the wave's pixel tiles 2 s and 2 s + 1.  At KT = 2 pass 1
  // uses four slots of a buffer, one fragment of each of the four tiles.
  bf16x8 bq[NB][6];
  const auto bload = [&](bf16x8 (&d)[6], int s, int o0, int o1, int o2) __attribute__((always_inline)) {
#pragma unroll
    for (int ptl = 0; ptl < 2; ++ptl) {
      d[3 * ptl + 0] = *reinterpret_cast<const bf16x8*>(lds + pbase + ((2 * s + ptl) * PT_BYTES + o0));
      d[3 * ptl + 1] = *reinterpret_cast<const bf16x8*>(lds + pbase + ((2 * s + ptl) * PT_BYTES + o1));
      d[3 * ptl + 2] = *reinterpret_cast<const bf16x8*>(lds + pbase + ((2 * s + ptl) * PT_BYTES + o2));
    }
  };
  const auto mfma = [](const bf16x8& a, const bf16x8& b, const f32x16& c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  };

  for (int cb = 0; cb < C; cb += CB) {
    if (cb) __syncthreads();  // every wave is done with the previous block's planes
    // ---- stage: 8 channels of one halo pixel per item, split, one 16-byte store per plane
    // Three items at a time: their 24 loads go out together, ahead of a scheduling barrier, and are split and stored behind
    // it (all 48: spills at KT = 2).  The loads are unconditional: the channel is clamped to C - 1 and the pixel to the
    // plane's first, so every address lies inside x, and zero is selected afterwards (a guarded load is a branch of its own).
    // Items past the last one (the final trip's tail) load item 0's addresses and store nothing.  Offsets within a sample
    // fit 32 bits (C H W <= INT_MAX, host-checked).
    constexpr int NIT = (4 * G::NPIX + NT - 1) / NT, GRP = 3;
    static_assert(NIT % GRP == 0, "staging items per thread come in whole groups");
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += GRP) {
      float v[GRP][8];
      int at[GRP], cfirst[GRP];  // LDS byte offset of the item (-1: store nothing) and its first channel (C: all zeros)
#pragma unroll
      for (int u = 0; u < GRP; ++u) {
        const int i_raw = tid + (it0 + u) * NT;
        const bool live = i_raw < 4 * G::NPIX;
        const int i = live ? i_raw : 0;
        const int g = i / G::NPIX, pix = i - g * G::NPIX;
        const int row = pix / G::HW, col = pix - row * G::HW;
        const int gh = h0 - 1 + row, gw = w0 - 1 + col;
        const bool inb = gh >= 0 && gh < H && gw >= 0 && gw < W;
        const int c0 = cb + 8 * g;
        const unsigned poff = inb ? gh * W + gw : 0;
        at[u] = live ? pix * PIX_BYTES + g * 16 : -1;
        cfirst[u] = inb ? c0 : C;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u][e] = xn[(unsigned)min(c0 + e, C - 1) * HWu + poff];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < GRP; ++u) {
        bf16x8 o[3];
        split8([&](int e) { return cfirst[u] + e < C ? v[u][e] : 0.f; }, o);
        if (at[u] >= 0) {
#pragma unroll
          for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(lds + at[u] + p * PLANE_BYTES) = o[p];
        }
      }
    }
    __syncthreads();
    // ---- multiply: two passes of 9 taps x 2 k-steps; weight fragments from L2, pixel fragments from LDS, 6 PT MFMAs per step
    f32x16 acc[PT];
    acc_zero(acc);
    // The block after this one, whose first unit the last trip requests.  After the last block there is none: the pointer is
    // CLAMPED to this block, whose first unit is loaded once more and dropped -- no address outside `packed` is formed.
    const bf16x8* const wnext = cb + CB < C ? wblk + 2 * 64 : wblk;
    // the first unit's pixel fragments: the one LDS fetch that nothing covers
#pragma unroll
    for (int s = 0; s < NH; ++s) bload(bq[s], s, 0, PLANE_BYTES, 2 * PLANE_BYTES);
    // pass 0: the five small products of every tap and step, while the accumulator is small (their roundings are 2^-8 of the
    // block's sum).  A unit is one (tap, step): three planes of weights, and of pixels per pixel tile, 5 PT MFMAs, taken in
    // NH halves of two pixel tiles.  The next unit's weights are requested before the unit's first MFMAs, and behind the
    // first MFMAs of every half the same half of the next unit: NH halves ahead, into the ring's free buffer.
#pragma unroll 1  // a row of taps per trip: unrolled further, the scheduler hoists pass 1's loads until registers spill
    for (int trow = 0; trow < 3; ++trow) {
      const long wrow = 3 * trow * tap_frags;
      pin_wl();
      const int brow = trow * G::HW * PIX_BYTES;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        constexpr int PA[5] = {2, 1, 0, 1, 0}, PB[5] = {0, 1, 2, 0, 1};  // (weight plane, input plane), smallest product first
        const bool more = trow < 2;  // j == 5: the next row's first unit, else pass 1's first fragments
#pragma unroll
        for (int s = 0; s < NH; ++s) {
          bf16x8(&cur)[6] = bq[(NH * j + s) % NB];
          bf16x8(&nxt)[6] = bq[(NH * j + s + NH) % NB];  // 6 NH halves per trip, a multiple of NB: the indices are static
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
          if (s == 0) {
            if (j < 5) {
              const long o = wrow + ((j + 1) >> 1) * tap_frags + ((j + 1) & 1) * 64;
              wload(wq[(j + 1) & 1], wblk, o, o + plane_frags, o + 2 * plane_frags);
            } else {  // pass 1 starts with plane 0 of units 0..2
              const long o = wrow + 3 * tap_frags;
              wload(wq[0], wblk, more ? o : 0, more ? o + plane_frags : 64, more ? o + 2 * plane_frags : tap_frags);
            }
            __builtin_amdgcn_sched_barrier(SCHED_FREE);
          }
#pragma unroll
          for (int ptl = 0; ptl < 2; ++ptl)
            acc[2 * s + ptl] = mfma(wq[j & 1][PA[0]], cur[3 * ptl + PB[0]], acc[2 * s + ptl]);
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
          if (j < 5) {
            const int o = brow + ((j + 1) >> 1) * PIX_BYTES + ((j + 1) & 1) * 32;
            bload(nxt, s, o, o + PLANE_BYTES, o + 2 * PLANE_BYTES);
          } else if constexpr (KT == 1) {  // pass 1's first group: plane 0 of units 0..2
            const int o = brow + G::HW * PIX_BYTES;
            bload(nxt, 0, more ? o : 0, more ? o + PLANE_BYTES : 32, more ? o + 2 * PLANE_BYTES : PIX_BYTES);
          } else {  // pass 1's unit s: plane 0 of (tap 0, step s) for the four pixel tiles; slots 4 and 5 are not used there
            const int o = brow + G::HW * PIX_BYTES;
#pragma unroll
            for (int i = 0; i < 6; ++i)
              nxt[i] = *reinterpret_cast<const bf16x8*>(
                  lds + pbase + (more ? (2 * s + i / 3) * PT_BYTES + o + (i % 3) * PLANE_BYTES : (i & 3) * PT_BYTES + 32 * s));
          }
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
#pragma unroll
          for (int q = 1; q < 5; ++q)
#pragma unroll
            for (int ptl = 0; ptl < 2; ++ptl)
              acc[2 * s + ptl] = mfma(wq[j & 1][PA[q]], cur[3 * ptl + PB[q]], acc[2 * s + ptl]);
        }
      }
    }
    // pass 1: the (w0, x0) products on top -- 18 roundings at the block's magnitude instead of 108.  A unit is PT MFMAs,
    // shorter than a load takes.  The weights are requested three units at a time (a buffer holds plane 0 of three
    // consecutive units), so that three to six are in flight.
    if constexpr (KT == 1) {  // the pixel fragments likewise: a buffer holds three units of both tiles
#pragma unroll 1
      for (int trow = 0; trow < 3; ++trow) {
        const long wrow = 3 * trow * tap_frags;
        pin_wl();
        const int brow = trow * G::HW * PIX_BYTES;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const bool more = trow < 2;  // g == 1: units 0..2 of the next row, else the next block's first unit of pass 0 (wnext)
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
          if (g == 0) {  // units 3..5 of this row: (tap 1, step 1), (2, 0), (2, 1)
            wload(wq[1], wblk, wrow + tap_frags + 64, wrow + 2 * tap_frags, wrow + 2 * tap_frags + 64);
          } else {
            const long o = wrow + 3 * tap_frags;
            wload(wq[0], more ? wblk : wnext, more ? o : 0, more ? o + 64 : plane_frags, more ? o + tap_frags : 2 * plane_frags);
          }
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
#pragma unroll
          for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) acc[pt] = mfma(wq[g][p], bq[g][3 * pt + p], acc[pt]);
            if (p == 0) {
              __builtin_amdgcn_sched_barrier(SCHED_FREE);
              if (g == 0) {
                bload(bq[1], 0, brow + PIX_BYTES + 32, brow + 2 * PIX_BYTES, brow + 2 * PIX_BYTES + 32);
              } else {  // after the last row the next block is not staged yet: this row's fragments are read again and dropped
                const int o = more ? brow + G::HW * PIX_BYTES : brow;
                bload(bq[0], 0, o, o + 32, o + PIX_BYTES);
              }
              __builtin_amdgcn_sched_barrier(SCHED_FREE);
            }
          }
        }
      }
    } else {  // one unit's four pixel fragments per buffer (slots 0..3), two units ahead in the ring of three
      const auto bload4 = [&](bf16x8 (&d)[6], int o) __attribute__((always_inline)) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) d[pt] = *reinterpret_cast<const bf16x8*>(lds + pbase + (pt * PT_BYTES + o));
      };
#pragma unroll 1
      for (int trow = 0; trow < 3; ++trow) {
        const long wrow = 3 * trow * tap_frags;
        pin_wl();
        const int brow = trow * G::HW * PIX_BYTES;
#pragma unroll
        for (int u = 0; u < 6; ++u) {  // unit u = (tap u >> 1, step u & 1): weights wq[u / 3][u % 3], pixels bq[u % 3]
          const bool more = trow < 2;  // u >= 3: units 0..2 of the next row, else the next block's first unit of pass 0 (wnext)
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
          if (u == 0) {  // units 3..5 of this row: (tap 1, step 1), (2, 0), (2, 1)
            wload(wq[1], wblk, wrow + tap_frags + 64, wrow + 2 * tap_frags, wrow + 2 * tap_frags + 64);
            __builtin_amdgcn_sched_barrier(SCHED_FREE);
          } else if (u == 3) {
            const long o = wrow + 3 * tap_frags;
            wload(wq[0], more ? wblk : wnext, more ? o : 0, more ? o + 64 : plane_frags, more ? o + tap_frags : 2 * plane_frags);
            __builtin_amdgcn_sched_barrier(SCHED_FREE);
          }
          acc[0] = mfma(wq[u / 3][u % 3], bq[u % 3][0], acc[0]);
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
          if (u < 4) {
            bload4(bq[(u + 2) % 3], brow + ((u + 2) >> 1) * PIX_BYTES + ((u + 2) & 1) * 32);
          } else {  // after the last row the next block is not staged yet: this row's fragments are read again and dropped
            bload4(bq[(u + 2) % 3], (more ? brow + G::HW * PIX_BYTES : brow) + (u & 1) * 32);
          }
          __builtin_amdgcn_sched_barrier(SCHED_FREE);
#pragma unroll
          for (int pt = 1; pt < 4; ++pt) acc[pt] = mfma(wq[u / 3][u % 3], bq[u % 3][pt], acc[pt]);
        }
      }
    }
    wblk = wnext;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) tot[pt] = tot[pt] + acc[pt];
  }
  // ---- store: accumulator register i of lane (r, hh) is output channel acc_channel(i, hh) of its tile, pixel r
  // act: the dense estimator's epilogue, bias_act_fwd_kernel's arithmetic (v += b; v > 0 ? v : v * slope), applied to the
  // totals in registers under ONE uniform branch, the bias index clamped so that the lane's 16 loads need no guard and go
  // out together.  (One branch and one guarded load per store cost every call 1.7 %, with or without the epilogue.)
  if (act) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = 32 * ktw + acc_channel(i, hh);
      const float b = bias ? bias[k < K ? k : K - 1] : 0.f;
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        float v = tot[pt][i];
        v += b;
        tot[pt][i] = v > 0.f ? v : v * slope;
      }
    }
  }
  float* yn = y + (long)n * y_bs;
  const int gw = w0 + pcol;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int gh = h0 + prow0 + pt * G::PR;
    if (gh >= H || gw >= W) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = 32 * ktw + acc_channel(i, hh);
      if (k < K) yn[(long)k * HWl + gh * W + gw] = tot[pt][i];
    }
  }
}

inline bool pack_shape_ok(int K, int C) {
  return K > 0 && C > 0 && (long)K * C * 9 <= INT_MAX && (long)9 * tiles32(K) * 2 * tiles32(C) * 64 <= INT_MAX / 8;
}

struct Ends {  // where the input and the output live, and what the store does
  const float* x;
  long x_bs;
  float* y;
  long y_bs;
  const float* bias;
  int act;
  float slope;
};

template <int KT, int PW>
int launch(const Ends& ends, const bf16x8* packed, int N, int C, int K, int H, int W, int kt_first, int chunks, hipStream_t st) {
  using G = Geo<PW>;
  if (const int rc = allow_dynamic_lds<&splitconv_kernel<KT, PW>>(G::LDS_BYTES)) return rc;
  const int tx = (W + PW - 1) / PW, ty = (H + G::TH - 1) / G::TH;
  const dim3 grid((unsigned)((long)N * tx * ty), (unsigned)chunks);
  hipLaunchKernelGGL((splitconv_kernel<KT, PW>), grid, dim3(NT), G::LDS_BYTES, st, ends.x, ends.x_bs, packed, ends.y, ends.y_bs, ends.bias,
                     ends.act, ends.slope, C, K, H, W, tiles32(K), 2 * tiles32(C), kt_first, tx, ty);
  return af_launch_status();
}

template <int PW>
int launch_kt(int KT, const Ends& e, const bf16x8* packed, int N, int C, int K, int H, int W, int kt_first, int chunks,
              hipStream_t st) {
  return KT == 1 ? launch<1, PW>(e, packed, N, C, K, H, W, kt_first, chunks, st)
                 : launch<2, PW>(e, packed, N, C, K, H, W, kt_first, chunks, st);
}
}  // namespace

extern "C" long arflow_splitconv_pack_bytes(int K, int C) {
  if (!pack_shape_ok(K, C)) return ARFLOW_ESHAPE;
  return (long)3 * 9 * tiles32(K) * 2 * tiles32(C) * FRAG * 2;
}

extern "C" int arflow_splitconv_pack(const float* w, void* packed, int K, int C, int transpose_flip, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(w);
  AF_REQUIRE_PTR(packed);
  AF_REQUIRE(pack_shape_ok(K, C), ARFLOW_ESHAPE);
  AF_REQUIRE(transpose_flip == 0 || transpose_flip == 1, ARFLOW_EPARAM);
  AF_REQUIRE(((uintptr_t)packed & 15) == 0, ARFLOW_EPARAM);
  const int Kout = transpose_flip ? C : K, Cin = transpose_flip ? K : C;
  const int nkt = tiles32(Kout), ncs = 2 * tiles32(Cin);
  const int nfrag = 9 * nkt * ncs * 64;
  hipLaunchKernelGGL(splitconv_pack_kernel, dim3((unsigned)af_cdiv(nfrag, NT)), dim3(NT), 0, (hipStream_t)stream, w,
                     (bf16x8*)packed, K, C, Kout, Cin, nkt, ncs, transpose_flip);
  return af_launch_status();
}

extern "C" int arflow_splitconv_fwd_ex(const float* x, long x_bstride, const void* packed, float* y, long y_bstride,
                                       const float* bias, int act, float negative_slope, int N, int C, int K, int H, int W,
                                       arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(x);
  AF_REQUIRE_PTR(packed);
  AF_REQUIRE_PTR(y);
  AF_REQUIRE(N > 0 && C > 0 && K > 0 && H > 0 && W > 0, ARFLOW_ESHAPE);
  AF_REQUIRE((long)N * C * H * W <= INT_MAX && (long)N * K * H * W <= INT_MAX && pack_shape_ok(K, C), ARFLOW_ESHAPE);
  AF_REQUIRE(x_bstride >= (long)C * H * W && y_bstride >= (long)K * H * W, ARFLOW_ESHAPE);
  AF_REQUIRE(x_bstride <= INT_MAX / N && y_bstride <= INT_MAX / N, ARFLOW_ESHAPE);  // N * stride within INT_MAX
  AF_REQUIRE(act == 0 || act == 1, ARFLOW_EPARAM);
  AF_REQUIRE(act == 1 || bias == nullptr, ARFLOW_EPARAM);
  AF_REQUIRE(((uintptr_t)packed & 15) == 0, ARFLOW_EPARAM);
  const Ends ends{x, x_bstride, y, y_bstride, bias, act, negative_slope};
  const int PW = pixel_tile_width(H, W);  // split_tiles.hpp
  const bf16x8* pk = (const bf16x8*)packed;
  hipStream_t st = (hipStream_t)stream;
  for (const TilePart& p : split_tiles(tiles32(K), MAX_KT)) {  // one launch per part: chunks over gridDim.y
    if (p.count == 0) continue;
    int rc;
    if (PW == 32) rc = launch_kt<32>(p.kt, ends, pk, N, C, K, H, W, p.first, p.count, st);
    else if (PW == 16) rc = launch_kt<16>(p.kt, ends, pk, N, C, K, H, W, p.first, p.count, st);
    else rc = launch_kt<8>(p.kt, ends, pk, N, C, K, H, W, p.first, p.count, st);
    if (rc != ARFLOW_OK) return rc;
  }
  return ARFLOW_OK;
}

extern "C" int arflow_splitconv_fwd(const float* x, const void* packed, float* y, int N, int C, int K, int H, int W,
                                    arflow_stream_t stream) {
  // packed strides, plain store
  return arflow_splitconv_fwd_ex(x, (long)C * H * W, packed, y, (long)K * H * W, nullptr, 0, 0.f, N, C, K, H, W, stream);
}
