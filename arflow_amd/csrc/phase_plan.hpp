// The phase-mosaic layout of a dilated 3x3 convolution, stated once: phase.hip moves tensors by these
// maps and tests/phase_plan_check.cpp walks them on the CPU.  Plain C++ apart from the __host__ __device__ mark.
//
// A 3x3 convolution with dilation d and padding d is d * d independent dilation-1 / padding-1 convolutions, one per phase
// (p, q) on x[:, :, p::d, q::d].  Pg x Qg phase images (Pg | d, Qg | d) lie side by side in one VIRTUAL image with one row /
// column of zeros between neighbours -- the separator is both neighbours' zero padding, the image's border padding is the
// kernel's -- and the d * d / (Pg Qg) groups of a sample become samples of the virtual batch:
//     cell   Hs = ceil(H / d), Ws = ceil(W / d)
//     image  Hv = Pg (Hs + 1) - 1, Wv = Qg (Ws + 1) - 1,   batch Nv = N d d / (Pg Qg)
//     real (n, h, w), p = h % d, q = w % d  ->  n' = (n (d / Pg) + p / Pg) (d / Qg) + q / Qg,
//                                               hv = (p % Pg) (Hs + 1) + h / d,  wv = (q % Qg) (Ws + 1) + w / d
// A virtual element is a SEPARATOR (hv % (Hs + 1) == Hs or wv % (Ws + 1) == Ws), a RAGGED TAIL (its real row or column lies
// past H or W: the phases p >= H % d have one row less when d does not divide H) or real.  d = 1 is the identity: NCHW.
// The channel axis is not touched: a tensor [N, C, H, W] becomes [Nv, C, Hv, Wv], dense.
#pragma once
#include <climits>

#include "split_tiles.hpp"

#if defined(__HIPCC__)
#define PHASE_HD __host__ __device__
#else
#define PHASE_HD
#endif

namespace phase_plan {
struct Plan {
  int N, H, W, d;
  int Pg, Qg;  // phases per virtual image, down and across
  int Hs, Ws;  // cell
  int Hv, Wv, Nv;
};

inline bool shape_ok(int N, int H, int W, int d) { return N > 0 && H > 0 && W > 0 && d > 0 && d <= H && d <= W && (long)N * d * d <= INT_MAX; }

inline Plan with_groups(int N, int H, int W, int d, int Pg, int Qg) {
  Plan p;
  p.N = N, p.H = H, p.W = W, p.d = d, p.Pg = Pg, p.Qg = Qg;
  p.Hs = (H + d - 1) / d, p.Ws = (W + d - 1) / d;
  p.Hv = Pg * (p.Hs + 1) - 1, p.Wv = Qg * (p.Ws + 1) - 1;
  p.Nv = N * (d / Pg) * (d / Qg);
  return p;
}
// what the forward kernel pays for the virtual batch under its own tile rule, per real sample
inline long tiled_pixels(const Plan& p) {
  return (long)(p.d / p.Pg) * (p.d / p.Qg) * splitbf16::tile_pixels(p.Hv, p.Wv, splitbf16::pixel_tile_width(p.Hv, p.Wv));
}
// The mosaic: the divisor pair with the most real pixels per tile-rounded virtual pixel, i.e. the fewest tiled pixels; ties go
// to the smaller group (fewer separators), then to the smaller Pg.  The caller has checked shape_ok.
inline Plan make_plan(int N, int H, int W, int d) {
  Plan best = with_groups(N, H, W, d, 1, 1);
  for (int Pg = 1; Pg <= d; ++Pg) {
    if (d % Pg) continue;
    for (int Qg = 1; Qg <= d; ++Qg) {
      if (d % Qg) continue;
      const Plan c = with_groups(N, H, W, d, Pg, Qg);
      const long cc = tiled_pixels(c), cb = tiled_pixels(best);
      if (cc < cb || (cc == cb && Pg * Qg < best.Pg * best.Qg)) best = c;
    }
  }
  return best;
}
inline long elements(const Plan& p, int C) { return (long)p.Nv * C * p.Hv * p.Wv; }

// ---- the maps, one axis at a time (the kernels work on rows) ----
struct Row {   // where a real row h lives
  int g, hv;   // group of row phases p / Pg, virtual row
};
PHASE_HD inline Row row_to_virtual(const Plan& p, int h) {
  const int ph = h % p.d;
  return {ph / p.Pg, (ph % p.Pg) * (p.Hs + 1) + h / p.d};
}
struct Col {
  int g, wv;
};
PHASE_HD inline Col col_to_virtual(const Plan& p, int w) {
  const int ph = w % p.d;
  return {ph / p.Qg, (ph % p.Qg) * (p.Ws + 1) + w / p.d};
}
// the real row of virtual row hv in row group g, or -1: a separator or a ragged tail
PHASE_HD inline int row_to_real(const Plan& p, int g, int hv) {
  const int a = hv / (p.Hs + 1), i = hv % (p.Hs + 1);
  const int h = i * p.d + g * p.Pg + a;
  return i < p.Hs && h < p.H ? h : -1;
}
PHASE_HD inline int col_to_real(const Plan& p, int g, int wv) {
  const int b = wv / (p.Ws + 1), j = wv % (p.Ws + 1);
  const int w = j * p.d + g * p.Qg + b;
  return j < p.Ws && w < p.W ? w : -1;
}
// virtual sample of real sample n, row group gp, column group gq -- and back
PHASE_HD inline int sample_to_virtual(const Plan& p, int n, int gp, int gq) { return (n * (p.d / p.Pg) + gp) * (p.d / p.Qg) + gq; }

struct Pos {
  int n, h, w;
};
PHASE_HD inline Pos to_virtual(const Plan& p, int n, int h, int w) {
  const Row r = row_to_virtual(p, h);
  const Col c = col_to_virtual(p, w);
  return {sample_to_virtual(p, n, r.g, c.g), r.hv, c.wv};
}
// real position of a virtual element; false (o untouched) at a separator or a ragged tail
PHASE_HD inline bool to_real(const Plan& p, int nv, int hv, int wv, Pos& o) {
  const int nq = p.d / p.Qg, np = p.d / p.Pg;
  const int h = row_to_real(p, (nv / nq) % np, hv), w = col_to_real(p, nv % nq, wv);
  if (h < 0 || w < 0) return false;
  o = {nv / (nq * np), h, w};
  return true;
}
}  // namespace phase_plan
