// The launch plan of splitconv_wgrad.hip: strips, row blocks, the parts of the two channel axes, and
// the decode of a block id -- XCD remap included -- into what the workgroup owns.  Plain C++ apart from the
// __host__ __device__ mark, so that tests/wgrad_plan_check.cpp enumerates every block of a launch on the CPU.
#pragma once
#include <climits>

#include "split_tiles.hpp"

#if defined(__HIPCC__)
#define WGRAD_HD __host__ __device__
#else
#define WGRAD_HD
#endif

namespace wgrad_plan {
using splitbf16::MAX_KT;
using splitbf16::split_tiles;
using splitbf16::tiles32;

constexpr int G = 8;           // groups of 8 pixels per staged row: 4 MFMA steps
constexpr int MAX_CT = 2;      // tiles of 32 input channels per workgroup (the kernel's template CT: 1 or 2)
constexpr int MAX_ROWS = 128;  // rows per chunk: the length of the running total's chain
constexpr int MIN_ROWS = 4;    // below that the two extra x rows a chunk stages dominate
constexpr int NCU = 256;
constexpr int NXCD = 8;        // block ids are dealt round-robin over the 8 XCDs, each with an L2 of its own

struct Plan {
  int GW, SG, nstrips, RPC, nrb, nct, nkt;
  int kt, kchunks;  // the kernel's KT -- min(nkt, 2): a single output-channel tile keeps the small workgroup -- and the chunks
  long chunks;
};
inline bool shape_ok(int N, int C, int K, int H, int W) {
  return N > 0 && C > 0 && K > 0 && H > 0 && W > 0 && (long)N * C * H * W <= INT_MAX && (long)N * K * H * W <= INT_MAX &&
         (long)9 * K * C <= INT_MAX;
}
// The kernel's CT.  Pairs of input-channel tiles only next to pairs of output-channel tiles: <KT 1, CT 2> is one workgroup
// of six waves per CU and measured slower than two of <1, 1>.  vec: the float4 staging loads; without them the 2 x 2
// workgroup does not fit 168 registers (60 bytes of scratch) and is not built.
constexpr int plan_ct(int kt, bool vec) { return kt == MAX_KT && vec ? MAX_CT : 1; }
inline Plan make_plan(int N, int C, int K, int H, int W) {
  Plan p;
  p.GW = (W + 7) / 8;
  const int ns = (p.GW + G - 1) / G;
  p.SG = 2 * ((p.GW + 2 * ns - 1) / (2 * ns));  // strips of equal, even width (a step is two groups), at most G
  p.nstrips = (p.GW + p.SG - 1) / p.SG;
  p.nct = tiles32(C), p.nkt = tiles32(K);
  p.kt = p.nkt < MAX_KT ? p.nkt : MAX_KT, p.kchunks = (p.nkt + MAX_KT - 1) / MAX_KT;
  // workgroups as the float4 kernel cuts them, against the workgroups a CU holds (one of 2 x 2 tiles, else two), twice over.
  // The chunks must not depend on the alignment of the pointers: arflow_splitconv_wgrad_ws_bytes does not see them.
  const int ct = plan_ct(p.kt, true);
  const long units = (long)((p.nct + ct - 1) / ct) * p.kchunks * N * p.nstrips;
  const long want_wg = 2 * NCU * (ct == MAX_CT ? 1 : 2);
  const long want = (want_wg + units - 1) / units;  // row blocks that fill the chip
  int rpc = (int)((H + want - 1) / want);
  if (rpc < MIN_ROWS) rpc = MIN_ROWS;
  if (rpc > MAX_ROWS) rpc = MAX_ROWS;
  if (rpc > H) rpc = H;
  p.RPC = rpc;
  p.nrb = (H + rpc - 1) / rpc;
  p.chunks = (long)N * p.nstrips * p.nrb;
  return p;
}
inline long ws_bytes(const Plan& p, int K, int C) { return p.chunks * 9 * K * C * 4; }

// The one launch of a call: every chunk times every output-channel part times every input-channel part.  Both channel axes
// are cut as split_tiles cuts them -- `extra` parts of base + 1 tiles, then parts of base tiles; no tile of zeros is
// multiplied: the waves of a part one tile short of the kernel's KT or CT have no tile and only stage.
struct Launch {
  int kt, kparts, kbase, kextra;  // the kernel's KT (the largest part), the parts and their sizes
  int ct, cparts, cbase, cextra;
  int nstrips, nrb;
  long blocks;
};
inline Launch make_launch(const Plan& p, bool vec) {
  Launch l;
  const auto k = split_tiles(p.nkt, MAX_KT), c = split_tiles(p.nct, plan_ct(p.kt, vec));
  l.kt = p.kt, l.kparts = k[0].count + k[1].count, l.kbase = k[1].kt, l.kextra = k[0].count;
  l.ct = c[0].count ? c[0].kt : c[1].kt, l.cparts = c[0].count + c[1].count, l.cbase = c[1].kt, l.cextra = c[0].count;
  l.nstrips = p.nstrips, l.nrb = p.nrb;
  l.blocks = p.chunks * l.kparts * l.cparts;
  return l;
}

// Blocks whose ids are equal mod 8 share an XCD.  The remap gives each XCD a run of consecutive logical ids -- so the
// workgroups of one chunk, which share its dy rows and x tiles, sit behind one L2 -- and is a bijection of [0, nwg) for
// every nwg, a multiple of 8 or not.  A pure speed choice: which block computes what does not change any result.
WGRAD_HD inline unsigned xcd_remap(unsigned orig, unsigned nwg) {
  const unsigned q = nwg / NXCD, r = nwg % NXCD, x = orig % NXCD;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + orig / NXCD;
}

struct Block {
  int n, strip, rb, chunk;  // the chunk (sample, strip, row block) and its number
  int kt0, ktn;             // first output-channel tile and how many (<= the launch's kt)
  int ct0, ctn;             // first input-channel tile and how many (<= the launch's ct)
};
// logical id = (chunk, output-channel part, input-channel part), the input-channel part fastest
WGRAD_HD inline Block decode_block(unsigned block_id, unsigned nwg, const Launch& l) {
  const int b = (int)xcd_remap(block_id, nwg);
  const int cp = b % l.cparts, kp = (b / l.cparts) % l.kparts;
  Block o;
  o.chunk = b / (l.cparts * l.kparts);
  o.rb = o.chunk % l.nrb, o.strip = (o.chunk / l.nrb) % l.nstrips, o.n = o.chunk / (l.nrb * l.nstrips);
  o.kt0 = kp < l.kextra ? kp * (l.kbase + 1) : l.kextra * (l.kbase + 1) + (kp - l.kextra) * l.kbase;
  o.ktn = kp < l.kextra ? l.kbase + 1 : l.kbase;
  o.ct0 = cp < l.cextra ? cp * (l.cbase + 1) : l.cextra * (l.cbase + 1) + (cp - l.cextra) * l.cbase;
  o.ctn = cp < l.cextra ? l.cbase + 1 : l.cbase;
  return o;
}
// ws: [chunk][tap][K][C] partial sums
WGRAD_HD inline long ws_index(int chunk, int tap, int k, int c, int K, int C) { return (((long)chunk * 9 + tap) * K + k) * C + c; }
}  // namespace wgrad_plan
