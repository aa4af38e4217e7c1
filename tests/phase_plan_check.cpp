// Host check of the phase-mosaic layout (arflow_amd/csrc/phase_plan.hpp), built and run by
// tests/test_phase_plan_cpu.py.  For H, W in 1..70 plus 96 x 160 and 384 x 640 / 4, d in {1, 2, 4, 8, 16} (d <= H, W; the others
// must be refused) it asserts that
//   - every real pixel maps to exactly one virtual element, inside the virtual tensor, and back to itself;
//   - separators, ragged tails and real elements partition the virtual tensor (the real ones count N H W);
//   - the chosen mosaic has the fewest tile-rounded pixels of all divisor pairs -- the largest fill -- the smaller group on ties;
//   - d = 1 is the identity, and the sizes stay inside the INT_MAX guards.
// It prints the fill table of the flagship shape.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "phase_plan.hpp"

using namespace phase_plan;

static int gN, gH, gW, gd;
#define CHECK(cond)                                                                                            \
  do {                                                                                                         \
    if (!(cond)) {                                                                                             \
      std::fprintf(stderr, "%s:%d: %s  [N %d H %d W %d d %d]\n", __FILE__, __LINE__, #cond, gN, gH, gW, gd); \
      std::exit(1);                                                                                            \
    }                                                                                                          \
  } while (0)

static long checked = 0;

static void check_shape(int N, int H, int W, int d) {
  gN = N, gH = H, gW = W, gd = d;
  if (d > H || d > W) {
    CHECK(!shape_ok(N, H, W, d));
    return;
  }
  CHECK(shape_ok(N, H, W, d));
  const Plan p = make_plan(N, H, W, d);
  ++checked;
  CHECK(d % p.Pg == 0 && d % p.Qg == 0 && p.Hs == (H + d - 1) / d && p.Ws == (W + d - 1) / d);
  CHECK(p.Hv == p.Pg * (p.Hs + 1) - 1 && p.Wv == p.Qg * (p.Ws + 1) - 1 && (long)p.Nv * p.Pg * p.Qg == (long)N * d * d);
  CHECK(elements(p, 640) <= (long)INT_MAX && (long)p.Nv * p.Hv * p.Wv > 0);
  if (d == 1) CHECK(p.Nv == N && p.Hv == H && p.Wv == W);
  // the choice: no divisor pair is cheaper, and none as cheap with a smaller group
  for (int Pg = 1; Pg <= d; ++Pg)
    for (int Qg = 1; Qg <= d; ++Qg) {
      if (d % Pg || d % Qg) continue;
      const Plan c = with_groups(N, H, W, d, Pg, Qg);
      CHECK(tiled_pixels(p) <= tiled_pixels(c));
      if (tiled_pixels(p) == tiled_pixels(c)) CHECK(p.Pg * p.Qg <= Pg * Qg);
    }
  // forward: each real pixel lands on its own virtual element, and comes back
  std::vector<unsigned char> hit((size_t)p.Nv * p.Hv * p.Wv, 0);
  for (int n = 0; n < N; ++n)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const Pos v = to_virtual(p, n, h, w);
        CHECK(v.n >= 0 && v.n < p.Nv && v.h >= 0 && v.h < p.Hv && v.w >= 0 && v.w < p.Wv);
        unsigned char& cell = hit[((size_t)v.n * p.Hv + v.h) * p.Wv + v.w];
        CHECK(!cell);
        cell = 1;
        Pos back{-1, -1, -1};
        CHECK(to_real(p, v.n, v.h, v.w, back) && back.n == n && back.h == h && back.w == w);
        if (d == 1) CHECK(v.n == n && v.h == h && v.w == w);
      }
  // backward: the virtual tensor is real elements + separators + tails, and nothing else
  long real = 0, sep = 0, tail = 0;
  for (int nv = 0; nv < p.Nv; ++nv)
    for (int hv = 0; hv < p.Hv; ++hv)
      for (int wv = 0; wv < p.Wv; ++wv) {
        Pos o{-1, -1, -1};
        const bool is_real = to_real(p, nv, hv, wv, o);
        const bool is_sep = hv % (p.Hs + 1) == p.Hs || wv % (p.Ws + 1) == p.Ws;
        CHECK(is_real == (hit[((size_t)nv * p.Hv + hv) * p.Wv + wv] != 0));
        CHECK(!(is_real && is_sep));
        if (is_real) {
          CHECK(o.n >= 0 && o.n < N && o.h >= 0 && o.h < H && o.w >= 0 && o.w < W);
          ++real;
        } else if (is_sep) {
          ++sep;
        } else {
          ++tail;  // a cell position whose real row or column lies past the map
          CHECK(H % d != 0 || W % d != 0);
        }
      }
  CHECK(real == (long)N * H * W && real + sep + tail == (long)p.Nv * p.Hv * p.Wv);
  if (H % d == 0 && W % d == 0) CHECK(tail == 0);
}

int main() {
  const int ds[] = {1, 2, 4, 8, 16};
  for (int d : ds) {
    for (int H = 1; H <= 70; ++H)
      for (int W = 1; W <= 70; ++W) check_shape(H % 3 + 1, H, W, d);
    check_shape(16, 96, 160, d);
    check_shape(2, 384 / 4, 640 / 4, d);
    check_shape(1, 384, 640, d);
  }
  // the guard itself: a batch whose virtual batch would pass INT_MAX is refused
  gN = INT_MAX / 128, gH = 96, gW = 160, gd = 16;
  CHECK(!shape_ok(INT_MAX / 128, 96, 160, 16));
  std::printf("phase plan ok: %ld layouts\n", checked);
  std::printf("fill at 16 x 96 x 160 (real pixels / tile-rounded virtual pixels):\n");
  for (int d : ds) {
    const Plan p = make_plan(16, 96, 160, d);
    std::printf("  d %2d  %2d x %2d  virtual %4d x %3d x %3d  PW %2d  fill %.1f %%\n", d, p.Pg, p.Qg, p.Nv, p.Hv, p.Wv,
                splitbf16::pixel_tile_width(p.Hv, p.Wv), 100.0 * 96 * 160 / (double)tiled_pixels(p));
  }
  return 0;
}
