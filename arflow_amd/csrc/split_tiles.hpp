// The cut of a channel axis into tiles of 32 and of the tiles into parts, shared by the split-bf16 convolution kernels
// (splitbf16.hpp) and by the weight gradient's launch plan (splitconv_wgrad_plan.hpp).  Plain C++: host tests compile it.
#pragma once
#include <array>

namespace splitbf16 {
inline int tiles32(int n) { return (n + 31) / 32; }
constexpr int MAX_KT = 2;  // tiles of 32 output channels per workgroup, in both kernels (their template KT: 1 or 2)

// n tiles of 32 channels go to the kernels in chunks of at most max_t tiles, of equal size +-1 (no tile of zeros is
// multiplied): `extra` chunks of base + 1 tiles, then the rest of base tiles.  count 0: none.
struct TilePart { int kt, count, first; };  // tiles per chunk, chunks, the first chunk's first tile
inline std::array<TilePart, 2> split_tiles(int n, int max_t) {
  const int chunks = (n + max_t - 1) / max_t, base = n / chunks, extra = n % chunks;
  return {{{base + 1, extra, 0}, {base, chunks - extra, extra * (base + 1)}}};
}

// The forward kernel's pixel tile: a workgroup owns 256 pixels as pw columns x 8 * (32 / pw) rows.  tile_pixels: the pixels an
// H x W map costs when it is cut into such tiles; pixel_tile_width: 32 x 1 where the rows are long enough, else 16 x 2 or 8 x 4
// (fewer columns of padding at W = 80, 40, 20).  The launcher (splitconv.hip) and the phase layout's choice of a mosaic
// (phase_plan.hpp) both ask here.
inline long tile_pixels(int H, int W, int pw) {
  const int th = 8 * (32 / pw);
  return (long)((W + pw - 1) / pw * pw) * ((H + th - 1) / th * th);
}
inline int pixel_tile_width(int H, int W) {
  int pw = 32;
  if (tile_pixels(H, W, 16) < tile_pixels(H, W, pw)) pw = 16;
  if (tile_pixels(H, W, 8) < tile_pixels(H, W, pw)) pw = 8;
  return pw;
}
}  // namespace splitbf16
