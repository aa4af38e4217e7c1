// What splitconv.hip (forward, data gradient) and splitconv_wgrad.hip (weight gradient) share: the exact
// split of an fp32 number into three bf16 planes, the MFMA accumulator layout, the cut of the output channels into launches.
// The ORDER of the six plane products is not here: it differs between the two on purpose, and each file header says why.
#pragma once
#include <array>

#include "common.hpp"
#include "split_tiles.hpp"

namespace splitbf16 {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// An fp32 number splits EXACTLY into three bf16 numbers, p[0] = bf16(x), p[1] = bf16(x - p[0]), p[2] = bf16(x - p[0] - p[1])
// (round to nearest even; both subtractions are exact): p[0] + p[1] + p[2] == x bit for bit.  This is the one definition
// tests/golden/splitconv_bits.txt and the accuracy tests rest on.
struct Split {
  __bf16 p[3];
  __device__ __forceinline__ explicit Split(float v) {
    p[0] = (__bf16)v;
    const float r1 = v - (float)p[0];
    p[1] = (__bf16)r1;
    p[2] = (__bf16)(r1 - (float)p[1]);
  }
};

// eight values -> their three planes, one 16-byte fragment each.  It takes value(e), not an array: a caller's guarded load or
// select stays inside the one loop (as a pass of its own ahead of the split it cost splitconv_pack_kernel 16 registers).
template <class F>
__device__ __forceinline__ void split8(const F& value, bf16x8 (&o)[3]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const Split s(value(e));
    o[0][e] = s.p[0], o[1][e] = s.p[1], o[2][e] = s.p[2];
  }
}

// v_mfma_f32_32x32x16_bf16: accumulator register i of lane (r = lane & 31, hh = lane >> 5) is row (i & 3) + 8 (i >> 2) + 4 hh
// of the 32 x 32 tile -- in both kernels the output channel within its tile -- and column r
__device__ __forceinline__ int acc_channel(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

__device__ __forceinline__ void acc_zero(f32x16& a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}
template <class T, int N>
__device__ __forceinline__ void acc_zero(T (&a)[N]) {  // an array of accumulators, of any rank
#pragma unroll
  for (int s = 0; s < N; ++s) acc_zero(a[s]);
}

// tiles32, MAX_KT, TilePart, split_tiles -- the cut of the output channels into launches -- are in split_tiles.hpp (host C++)

// more than 64 KB of dynamic LDS has to be asked for once per kernel: one flag per instantiation, i.e. per KERNEL
template <auto KERNEL>
inline int allow_dynamic_lds(int bytes) {
  static bool attr_set = false;
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return af_hip_status(e);
    attr_set = true;
  }
  return ARFLOW_OK;
}
}  // namespace splitbf16
