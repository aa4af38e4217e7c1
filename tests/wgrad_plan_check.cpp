// Host check of the weight gradient's launch plan (arflow_amd/csrc/splitconv_wgrad_plan.hpp), built
// and run by tests/test_splitconv_wgrad_plan_cpu.py.  For every shape of the sweep and both kinds of staging loads it walks
// every block id of the launch through the decode the kernel uses and asserts that
//   - the XCD remap is a bijection of the grid and hands each XCD one run of consecutive logical ids;
//   - every (chunk, output-channel tile, input-channel tile) is owned by exactly one workgroup, no tile outside the tensor;
//   - strips and row blocks tile the map, with at most MAX_ROWS rows per chunk;
//   - the workspace covers every store the kernel makes.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "splitconv_wgrad_plan.hpp"

using namespace wgrad_plan;

#define CHECK(cond)                                                                                                   \
  do {                                                                                                                \
    if (!(cond)) {                                                                                                    \
      std::fprintf(stderr, "%s:%d: %s  [N %d C %d K %d H %d W %d vec %d]\n", __FILE__, __LINE__, #cond, gN, gC, gK, gH, gW, gvec); \
      std::exit(1);                                                                                                   \
    }                                                                                                                 \
  } while (0)

static int gN, gC, gK, gH, gW, gvec;
static std::set<long> grids;

static void check_remap(unsigned nwg) {
  std::vector<unsigned char> seen(nwg, 0);
  std::vector<unsigned> lo(NXCD, ~0u), hi(NXCD, 0), cnt(NXCD, 0);
  for (unsigned b = 0; b < nwg; ++b) {
    const unsigned l = xcd_remap(b, nwg);
    CHECK(l < nwg && !seen[l]);
    seen[l] = 1;
    const unsigned x = b % NXCD;
    if (l < lo[x]) lo[x] = l;
    if (l > hi[x]) hi[x] = l;
    ++cnt[x];
    if (b >= NXCD) CHECK(l == xcd_remap(b - NXCD, nwg) + 1);  // an XCD's blocks take consecutive ids in dispatch order
  }
  for (int x = 0; x < NXCD; ++x) CHECK(cnt[x] == 0 || hi[x] - lo[x] + 1 == cnt[x]);
}

static void check_shape(int N, int C, int K, int H, int W, bool vec) {
  gN = N, gC = C, gK = K, gH = H, gW = W, gvec = vec;
  CHECK(shape_ok(N, C, K, H, W));
  const Plan p = make_plan(N, C, K, H, W);
  const long bytes = ws_bytes(p, K, C);
  CHECK(p.SG >= 2 && p.SG <= G && p.SG % 2 == 0 && p.nstrips * p.SG >= p.GW && (p.nstrips - 1) * p.SG < p.GW);
  CHECK(p.RPC >= 1 && p.RPC <= MAX_ROWS && p.nrb * p.RPC >= H && (p.nrb - 1) * p.RPC < H);
  CHECK(p.chunks == (long)N * p.nstrips * p.nrb && p.nct == tiles32(C) && p.nkt == tiles32(K));
  CHECK(p.kt >= 1 && p.kt <= MAX_KT && p.kchunks == (p.nkt + MAX_KT - 1) / MAX_KT);
  std::vector<unsigned char> owner((size_t)p.chunks * p.nkt * p.nct, 0);
  const Launch l = make_launch(p, vec);
  CHECK(l.kt == p.kt && l.kparts == p.kchunks && l.ct >= 1 && l.ct <= plan_ct(l.kt, vec));
  CHECK(l.blocks == p.chunks * l.kparts * l.cparts && l.blocks <= INT_MAX);
  grids.insert(l.blocks);
  check_remap((unsigned)l.blocks);
  for (unsigned b = 0; b < (unsigned)l.blocks; ++b) {
    const Block o = decode_block(b, (unsigned)l.blocks, l);
    CHECK(o.n >= 0 && o.n < N && o.strip >= 0 && o.strip < p.nstrips && o.rb >= 0 && o.rb < p.nrb);
    CHECK(o.chunk == (o.n * p.nstrips + o.strip) * p.nrb + o.rb && o.chunk < p.chunks);
    CHECK(o.rb * p.RPC < H && o.strip * p.SG < p.GW);
    CHECK(o.kt0 >= 0 && o.ktn >= 1 && o.ktn <= l.kt && o.kt0 + o.ktn <= p.nkt);
    CHECK(o.ct0 >= 0 && o.ctn >= 1 && o.ctn <= l.ct && o.ct0 + o.ctn <= p.nct);
    for (int kt = o.kt0; kt < o.kt0 + o.ktn; ++kt)
      for (int ct = o.ct0; ct < o.ct0 + o.ctn; ++ct) ++owner[((size_t)o.chunk * p.nkt + kt) * p.nct + ct];
    // the kernel stores taps 0..8 of channels k < min(K, 32 (kt0 + ktn)), c < min(C, 32 (ct0 + ctn)) of its tiles
    const int kmax = (32 * (o.kt0 + o.ktn) < K ? 32 * (o.kt0 + o.ktn) : K) - 1, cmax = (32 * (o.ct0 + o.ctn) < C ? 32 * (o.ct0 + o.ctn) : C) - 1;
    CHECK(kmax >= 32 * o.kt0 && cmax >= 32 * o.ct0);
    CHECK(ws_index(o.chunk, 0, 32 * o.kt0, 32 * o.ct0, K, C) >= 0 && (ws_index(o.chunk, 8, kmax, cmax, K, C) + 1) * 4 <= bytes);
  }
  for (unsigned char c : owner) CHECK(c == 1);
}

int main() {
  const int Ns[] = {1, 2, 16}, Cs[] = {1, 31, 32, 33, 64, 65, 96, 97, 147, 563, 597}, Hs[] = {1, 4, 5, 96}, Ws[] = {1, 8, 63, 64, 65, 160};
  long shapes = 0;
  for (int N : Ns)
    for (int C : Cs)
      for (int K : Cs)
        for (int H : Hs)
          for (int W : Ws)
            for (int vec = 0; vec < 2; ++vec) check_shape(N, C, K, H, W, vec), ++shapes;
  for (int N = 1; N <= 17; ++N)  // one workgroup per sample: grids of 1 .. 17 workgroups, around the 8 XCDs
    for (int vec = 0; vec < 2; ++vec) check_shape(N, 32, 32, 4, 8, vec), ++shapes;
  gN = gC = gK = gH = gW = gvec = 0;
  for (long g = 1; g <= 17; ++g) CHECK(grids.count(g));
  for (unsigned nwg = 1; nwg <= 4100; ++nwg) check_remap(nwg);
  std::printf("wgrad plan ok: %ld plans, %zu distinct grid sizes\n", shapes, grids.size());
  return 0;
}
