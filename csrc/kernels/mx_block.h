// What a kernel needs of one 32-element block of the `mxfp8_e4m3` format when the block's eight lanes sit next to
// each other in a wave64 (four f32 elements per lane): the block amax as a DPP butterfly, the scale rule on the f32
// bits, and the packed FP8 converts with the scale applied. mx_wire.hip (the wire kernels, every format) and
// adamw8.hip (the 8-bit optimizer state) read this one definition. Contract: docs/collectives.md "Compressed
// all-reduce".
#pragma once
#include "dev_common.h"

namespace pdcc {
namespace dev {

using F8 = Tr<DType::F8E4M3>;

// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror: lane ^ 1, lane ^ 2, 7 - lane (of 8)
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t x) {
  const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
  return x > y ? x : y;
}
// max over the LANES (1, 2, 4 or 8) aligned neighbours that share a block; every one of them is active
template <int LANES>
__device__ __forceinline__ uint32_t group_max(uint32_t x) {
  if constexpr (LANES >= 2) x = dpp_max<kDppXor1>(x);
  if constexpr (LANES >= 4) x = dpp_max<kDppXor2>(x);
  if constexpr (LANES >= 8) x = dpp_max<kDppHalfMirror>(x);  // (both quads hold their max by now)
  return x;
}

__device__ __forceinline__ uint32_t abs_bits(float f) { return __float_as_uint(f) & 0x7fffffffu; }

// Scale of a block from max |x| as f32 bits: the byte, 2^-e for the payload, and whether the
// payload is written as zeros (an all-zero block, or one that holds an inf / a NaN).
struct MxScale {
  uint32_t byte;
  float inv;
  bool blank;
};
// amax = m 2^k, 1 <= m < 2 (k = -127 for a subnormal: the clamp decides). With the format's largest
// magnitude (1 + SWITCH 2^-23) 2^BIAS, the smallest e with amax 2^-e <= that is k - BIAS for a mantissa
// field <= SWITCH and one more above; e is clamped to [EMIN, EMAX] (the four constants: MxFmt in mx_fmt.h).
template <int BIAS, uint32_t SWITCH, int EMIN, int EMAX>
__device__ __forceinline__ MxScale mx_scale_of(uint32_t amax) {
  int e = (int)(amax >> 23) - 127 - BIAS + ((amax & 0x7fffffu) > SWITCH ? 1 : 0);
  e = e < EMIN ? EMIN : (e > EMAX ? EMAX : e);
  const bool special = amax >= 0x7f800000u;
  if (amax == 0) e = 0;
  MxScale r;
  r.byte = special ? 255u : (uint32_t)(e + 127);
  r.inv = __uint_as_float((uint32_t)(127 - e) << 23);
  r.blank = special || amax == 0;
  return r;
}
// value of a scale byte: 2^(s - 127), NaN for 255 (0 would be the subnormal 2^-127; quantize never writes it)
__device__ __forceinline__ float mx_scale_value(uint32_t s) {
  return __uint_as_float(s == 255u ? 0x7fc00000u : (s == 0u ? 0x00400000u : s << 23));
}

__device__ __forceinline__ uint32_t narrow4(float a, float b, float c, float d, float inv) {
  return F8::narrow<true>(c * inv, d * inv, F8::narrow<false>(a * inv, b * inv, 0u));
}
__device__ __forceinline__ void widen4(uint32_t w, float scale, float* f) {
  const f32x2 lo = F8::widen<false>(w), hi = F8::widen<true>(w);
  f[0] = lo[0] * scale; f[1] = lo[1] * scale; f[2] = hi[0] * scale; f[3] = hi[1] * scale;
}

}  // namespace dev
}  // namespace pdcc
