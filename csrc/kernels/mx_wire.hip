// The local kernels of the block-scaled wire formats `mxfp8_e4m3`, `mxfp4_e2m1` and `mxfp6_e2m3` (layout:
// mx_layout.h, contract: docs/collectives.md "Compressed all-reduce", "Compressed reduce-scatter and
// all-gather", "The `mxfp4_e2m1` wire format" and "The `mxfp6_e2m3` wire format"):
//
//   mx_quantize    f32 / bf16 / f16 tensor -> wire           (reads 4n or 2n, writes 33n/32 or 17n/32)
//   mx_reduce      nsrc chunk wires -> one chunk wire         (dequantize, fold in f32, requantize)
//   mx_dequantize  wire -> f32 / bf16 / f16 tensor
//   mx_fold        nsrc chunk wires -> f32 / bf16 / f16 tensor (dequantize, fold in f32, round once)
//   mx_quantize_shards / mx_dequantize_shards: quantize / dequantize with one chunk per shard of m
//                  elements (the SHARD instantiations of the same two kernels)
//   mx_quantize_ef / mx_quantize_shards_ef / mx_reduce_ef: the EF instantiations of quantize and
//                  reduce, which add an f32 residual before they quantize and leave what the
//                  quantizer dropped in it (docs/collectives.md "Error feedback"); per f32 element
//                  quantize then reads 8 and writes 4 + 33/32 bytes instead of reading 4
//   mx_quantize_sr / mx_quantize_shards_sr / mx_reduce_sr: the SR instantiations of quantize and
//                  reduce, which round the payload stochastically (docs/collectives.md "Stochastic
//                  rounding", mx_sr.h); they move the bytes of the plain kernels
//
// All of them are streaming kernels: a lane moves 16 B on the wide side of its conversion (the tensor
// for quantize / dequantize / fold, the payload for reduce), the lanes of a block sit next to each other
// in a wave64, and a block's amax is a butterfly over those lanes with DPP moves -- no LDS, no
// atomics, no cross-workgroup traffic. A chunk is one grid row (blockIdx.y), so no lane divides by
// the chunk size.
//
// Numerics. amax and the scale exponent are integer work on the f32 bit patterns (|x| as an
// unsigned integer orders like |x|, and anything >= 0x7f800000 is an inf or a NaN). The scaling
// product x * 2^-e is one f32 multiply with subnormals kept (the default kernel mode), the
// narrowing is the packed convert the FP8 reductions use (nearest even), and 2^e never overflows
// or flushes: e is clamped to [-117, 120].
//
// Every kernel is a template over the format (MxFmt below): the formats share the lane layout on the
// tensor side and differ in the bytes a lane moves on the wire side (half as many for FP4), in the
// scale rule and in the packed converts. The FP4 payload goes through v_cvt_scalef32_pk_fp4_f32 /
// v_cvt_scalef32_pk_f32_fp4 with a unit scale operand: the product with 2^-e (2^e) is the same f32
// multiply as on the FP8 path, so the scale byte 255 -> NaN and the inf at the very top of the range
// come out of ordinary f32 arithmetic. e is clamped to [-125, 126] there.
//
// The FP6 payload is a bit stream: a lane's 4 or 8 codes are 24 or 48 bits, so on the tensor-side lane
// layout (quantize, dequantize, fold) the lanes of a quad (f32) or of a pair (bf16 / f16) own 96 bits = 3
// aligned dwords between them and trade the straddling bits with one DPP move; every payload access is
// an aligned dword and a wave's accesses are contiguous. Reduce takes a whole block per lane (24 bytes
// as three aligned 8-byte accesses), as FP4 does. The codes go through the FP8 converts: e2m3 is e4m3
// with the exponent field cut to two bits, so the e4m3 byte of s / 64 has bits 5 and 6 clear for
// |s| <= 7.5 and the code is its low five bits and its sign (MxFmt<FP6_E2M3> below). e is clamped to
// [-123, 126].
#include <algorithm>

#include "dev_common.h"
#include "mx_layout.h"
#include "mx_rot.h"
#include "mx_sr.h"

namespace pdcc {
namespace dev {

namespace {

using F8 = Tr<DType::F8E4M3>;
using kern::MxFormat;
constexpr int kMxUnroll = 4;  // independent 16-B loads in flight per lane (quantize / dequantize)

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

// ---- Hadamard rotation (mx_rot.h, docs/collectives.md "Hadamard rotation"). A lane holds the EPL elements
// from position `place * EPL` of its block, place = v % LPB. The butterfly stages below EPL pair elements
// of the lane, the later ones pair the lane with lane ^ 1, ^ 2 and (f32) ^ 4 of its block: quad_perm for
// the first two, row_shl:4 for the low and row_shr:4 for the high four lanes of the eight (row_half_mirror
// would pair i with 7 - i). The low lane of a pair keeps a + b and the high one a - b; as the sum of the
// partner's value and its own with the sign flipped that is one v_add_f32 whose operand comes through DPP.
// Every lane of the block must be active. Contraction is off inside: the order of the f32 roundings is the
// definition, also where a dequantized operand's product with its scale overflows.
constexpr int kDppRowShl4 = 0x104, kDppRowShr4 = 0x114;
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), CTRL, 0xf, 0xf, true));
}
template <int EPL>
__device__ __forceinline__ void rot_flip(float* f, uint32_t signs, uint32_t place) {
  const uint32_t s = signs >> (place * EPL);
#pragma unroll
  for (int i = 0; i < EPL; ++i) f[i] = __uint_as_float(__float_as_uint(f[i]) ^ ((s >> i) << 31));
}
// stage h = EPL * X of the butterfly: the exchange with lane ^ X
template <int EPL, int X>
__device__ __forceinline__ void rot_exchange(float* f, uint32_t place) {
#pragma clang fp contract(off)  // (one f32 add each: nothing fused with the product that made an operand)
  const bool high = (place & X) != 0;
  const uint32_t flip = high ? 0x80000000u : 0u;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    float p;
    if constexpr (X == 1) p = dpp_f32<kDppXor1>(f[i]);
    else if constexpr (X == 2) p = dpp_f32<kDppXor2>(f[i]);
    else {
      const float up = dpp_f32<kDppRowShl4>(f[i]), down = dpp_f32<kDppRowShr4>(f[i]);
      p = high ? down : up;
    }
    f[i] = p + __uint_as_float(__float_as_uint(f[i]) ^ flip);  // low: b + a, high: a - b
  }
}
template <int EPL>
__device__ __forceinline__ void rot_butterfly(float* f, uint32_t place) {
#pragma clang fp contract(off)
#pragma unroll
  for (int h = 1; h < EPL; h <<= 1) {
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      if ((j & h) == 0) {
        const float a = f[j], b = f[j + h];
        f[j] = a + b;
        f[j + h] = a - b;
      }
    }
  }
  rot_exchange<EPL, 1>(f, place);
  rot_exchange<EPL, 2>(f, place);
  if constexpr (EPL == 4) rot_exchange<EPL, 4>(f, place);
}
// R x: signs, then the butterfly
template <int EPL>
__device__ __forceinline__ void rot_forward(float* f, uint32_t signs, uint32_t place) {
  rot_flip<EPL>(f, signs, place);
  rot_butterfly<EPL>(f, place);
}
// R^-1 d: the butterfly, one multiply by 2^-5, then the signs
template <int EPL>
__device__ __forceinline__ void rot_inverse(float* f, uint32_t signs, uint32_t place) {
  rot_butterfly<EPL>(f, place);
#pragma unroll
  for (int i = 0; i < EPL; ++i) f[i] *= 0.03125f;
  rot_flip<EPL>(f, signs, place);
}

// Scale of a block from max |x| as f32 bits: the byte, 2^-e for the payload, and whether the
// payload is written as zeros (an all-zero block, or one that holds an inf / a NaN).
struct MxScale {
  uint32_t byte;
  float inv;
  bool blank;
};
__device__ __forceinline__ MxScale mx_scale(uint32_t amax) {
  // amax = m 2^k, 1 <= m < 2 (k = -127 for a subnormal: the clamp decides); the smallest e with
  // amax 2^-e <= 448 = 1.75 2^8 is k - 8 for m <= 1.75 and k - 7 above
  int e = (int)(amax >> 23) - 127 - 8 + ((amax & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < -117 ? -117 : (e > 120 ? 120 : e);
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

// e2m1: element 2j of a dword's eight sits in the low nibble of byte j, element 2j + 1 in the high one.
// The scale operand of the converts is 1: the kernels multiply in f32 (see the top of the file).
__device__ __forceinline__ uint32_t fp4_narrow4(float a, float b, float c, float d, float inv, uint32_t old, bool hi) {
  if (hi) {
    old = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, a * inv, b * inv, 1.0f, 2);
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, c * inv, d * inv, 1.0f, 3);
  }
  old = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, a * inv, b * inv, 1.0f, 0);
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, c * inv, d * inv, 1.0f, 1);
}
__device__ __forceinline__ void fp4_widen8(uint32_t w, float scale, float* f) {
  const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
  const f32x2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  const f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2);
  const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
  f[0] = a[0] * scale; f[1] = a[1] * scale; f[2] = b[0] * scale; f[3] = b[1] * scale;
  f[4] = c[0] * scale; f[5] = c[1] * scale; f[6] = d[0] * scale; f[7] = d[1] * scale;
}
__device__ __forceinline__ MxScale mx4_scale(uint32_t amax) {
  // the smallest e with amax 2^-e <= 6 = 1.5 2^2 is k - 2 for m <= 1.5 and k - 1 above; the lower
  // clamp keeps 0.5 2^e a normal f32, the upper one is never reached (k <= 127)
  int e = (int)(amax >> 23) - 127 - 2 + ((amax & 0x7fffffu) > 0x400000u ? 1 : 0);
  e = e < -125 ? -125 : (e > 126 ? 126 : e);
  const bool special = amax >= 0x7f800000u;
  if (amax == 0) e = 0;
  MxScale r;
  r.byte = special ? 255u : (uint32_t)(e + 127);
  r.inv = __uint_as_float((uint32_t)(127 - e) << 23);
  r.blank = special || amax == 0;
  return r;
}

__device__ __forceinline__ MxScale mx6_scale(uint32_t amax) {
  // the smallest e with amax 2^-e <= 7.5 = 1.875 2^2 is k - 2 for m <= 1.875 and k - 1 above; the lower
  // clamp keeps 0.125 2^e a normal f32, the upper one is never reached (k <= 127)
  int e = (int)(amax >> 23) - 127 - 2 + ((amax & 0x7fffffu) > 0x700000u ? 1 : 0);
  e = e < -123 ? -123 : (e > 126 ? 126 : e);
  const bool special = amax >= 0x7f800000u;
  if (amax == 0) e = 0;
  MxScale r;
  r.byte = special ? 255u : (uint32_t)(e + 127);
  r.inv = __uint_as_float((uint32_t)(127 - e) << 23);
  r.blank = special || amax == 0;
  return r;
}
// e2m3 through the FP8 converts. Four scaled values s / 64 -> four e4m3 bytes -> 24 bits of codes (element
// j in bits 6j .. 6j + 5), and back: 24 bits -> four e4m3 bytes -> four values of s / 64.
__device__ __forceinline__ uint32_t fp6_narrow4(float a, float b, float c, float d, float inv64) {
  const uint32_t w = narrow4(a, b, c, d, inv64);                      // bits 5 and 6 of every byte are clear
  const uint32_t c4 = (w & 0x1f1f1f1fu) | ((w >> 2) & 0x20202020u);  // the sign from bit 7 to bit 5
  return (c4 & 0x3fu) | ((c4 >> 2) & 0xfc0u) | ((c4 >> 4) & 0x3f000u) | ((c4 >> 6) & 0xfc0000u);
}
__device__ __forceinline__ void fp6_widen4(uint32_t k, float scale, float* f) {
  const uint32_t c4 = (k & 0x3fu) | ((k << 2) & 0x3f00u) | ((k << 4) & 0x3f0000u) | ((k << 6) & 0x3f000000u);
  const uint32_t w = (c4 & 0x1f1f1f1fu) | ((c4 & 0x20202020u) << 2);
  const f32x2 lo = F8::widen<false>(w), hi = F8::widen<true>(w);
  // value / 64 is exact in f32, so is the product with 64; 2^(e + 6) itself is no f32 for e > 121
  f[0] = lo[0] * 64.0f * scale; f[1] = lo[1] * 64.0f * scale; f[2] = hi[0] * 64.0f * scale; f[3] = hi[1] * 64.0f * scale;
}
// bits [pos, pos + n) of the little-endian bit stream held in the dwords q (pos and n constants, n <= 32)
__device__ __forceinline__ void bits_put(uint32_t* q, int pos, int n, uint32_t x) {
  const int w = pos / 32, o = pos % 32;
  q[w] |= x << o;
  if (o + n > 32) q[w + 1] |= x >> (32 - o);
}
__device__ __forceinline__ uint32_t bits_get(const uint32_t* q, int pos, int n) {
  const int w = pos / 32, o = pos % 32;
  uint32_t x = q[w] >> o;
  if (o + n > 32) x |= q[w + 1] << (32 - o);
  return x;  // (bits past n are the stream's next ones: the callers mask)
}

// What the kernels need of a format: payload bytes per block, the scale of a block, and N elements
// (4, 8, 16 or 32) to and from their N * kPayload / 32 payload bytes, held in dwords (kWords<N> of
// them; FP4 with N = 4 fills the low half of one). pack writes zeros for a blank block.
//
// kLanes: the payload of the tensor-side lanes (EPL = 4 or 8 elements) is no whole number of dwords, so
// the lanes that share 3 dwords exchange bits: ld_lanes (a lane's aligned dword loads), gather (the
// exchange that leaves the lane's own codes in q, called with every lower lane of the group active) and
// st_lanes (exchange and aligned dword stores, called with the whole group active) replace ld_wire / st_wire.
template <MxFormat F> struct MxFmt;
template <> struct MxFmt<MxFormat::FP8_E4M3> {
  static constexpr int kPayload = 32;
  static constexpr bool kLanes = false;
  template <int N> static constexpr int kWords = N / 4;
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx_scale(amax); }
  template <int N> __device__ static __forceinline__ void pack(const float* f, const MxScale& sc, uint32_t* q) {
#pragma unroll
    for (int d = 0; d < N / 4; ++d) {
      q[d] = narrow4(f[4 * d], f[4 * d + 1], f[4 * d + 2], f[4 * d + 3], sc.inv);
      if (sc.blank) q[d] = 0u;
    }
  }
  // stochastic rounding: element j takes the word `word(j)`; the integer rounding of mx_sr.h throughout
  template <int N, class W> __device__ static __forceinline__ void pack_sr(const float* f, const MxScale& sc, uint32_t* q,
                                                                          const W& word) {
#pragma unroll
    for (int d = 0; d < N / 4; ++d) {
      uint32_t w = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w |= kern::mx_sr_e4m3(__float_as_uint(f[4 * d + j] * sc.inv), word(4 * d + j)) << (8 * j);
      q[d] = sc.blank ? 0u : w;
    }
  }
  template <int N> __device__ static __forceinline__ void unpack(const uint32_t* q, float scale, float* f) {
#pragma unroll
    for (int d = 0; d < N / 4; ++d) widen4(q[d], scale, f + 4 * d);
  }
};
template <> struct MxFmt<MxFormat::FP4_E2M1> {
  static constexpr int kPayload = 16;
  static constexpr bool kLanes = false;
  template <int N> static constexpr int kWords = (N + 7) / 8;
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx4_scale(amax); }
  template <int N> __device__ static __forceinline__ void pack(const float* f, const MxScale& sc, uint32_t* q) {
#pragma unroll
    for (int d = 0; d < (N + 7) / 8; ++d) {
      q[d] = fp4_narrow4(f[8 * d], f[8 * d + 1], f[8 * d + 2], f[8 * d + 3], sc.inv, 0u, false);
      if constexpr (N >= 8) q[d] = fp4_narrow4(f[8 * d + 4], f[8 * d + 5], f[8 * d + 6], f[8 * d + 7], sc.inv, q[d], true);
      if (sc.blank) q[d] = 0u;
    }
  }
  template <int N, class W> __device__ static __forceinline__ void pack_sr(const float* f, const MxScale& sc, uint32_t* q,
                                                                          const W& word) {
    constexpr int G = N < 8 ? N : 8;  // elements of one dword
#pragma unroll
    for (int d = 0; d < (N + 7) / 8; ++d) {
      uint32_t w = 0u;
#pragma unroll
      for (int j = 0; j < G; ++j)
        w |= kern::mx_sr_e2m1(__float_as_uint(f[8 * d + j] * sc.inv), word(8 * d + j)) << (4 * j);
      q[d] = sc.blank ? 0u : w;
    }
  }
  template <int N> __device__ static __forceinline__ void unpack(const uint32_t* q, float scale, float* f) {
    if constexpr (N == 4) {
      float g[8];
      fp4_widen8(q[0], scale, g);
      f[0] = g[0]; f[1] = g[1]; f[2] = g[2]; f[3] = g[3];  // (the converts of the unused half fall away)
    } else {
#pragma unroll
      for (int d = 0; d < N / 8; ++d) fp4_widen8(q[d], scale, f + 8 * d);
    }
  }
};

// quad_perm [1,2,3,0], [0,0,1,2]: the next / the previous lane of a quad; [1,1,3,3], [0,0,2,2]: the odd /
// the even lane of a pair
constexpr int kDppQuadNext = 0x39, kDppQuadPrev = 0x90, kDppPairOdd = 0xF5, kDppPairEven = 0xA0;
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
template <> struct MxFmt<MxFormat::FP6_E2M3> {
  static constexpr int kPayload = 24;
  static constexpr bool kLanes = true;
  template <int N> static constexpr int kWords = (6 * N + 31) / 32;  // 4: 24 bits, 8: 48, 16: 96, 32: 192
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx6_scale(amax); }
  template <int N> __device__ static __forceinline__ void pack(const float* f, const MxScale& sc, uint32_t* q) {
    // 2^-(e + 6) from the scale byte e + 127: a subnormal for e > 120, where every |x| that does not round
    // to 0 still has a normal, exact product
    const int t = 248 - (int)sc.byte;
    const float inv64 = __uint_as_float(t >= 1 ? (uint32_t)t << 23 : 1u << (22 + (t < -22 ? -22 : t)));
#pragma unroll
    for (int d = 0; d < kWords<N>; ++d) q[d] = 0u;
#pragma unroll
    for (int g = 0; g < N / 4; ++g)
      bits_put(q, 24 * g, 24, fp6_narrow4(f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3], inv64));
    if (sc.blank) {
#pragma unroll
      for (int d = 0; d < kWords<N>; ++d) q[d] = 0u;
    }
  }
  template <int N, class W> __device__ static __forceinline__ void pack_sr(const float* f, const MxScale& sc, uint32_t* q,
                                                                          const W& word) {
#pragma unroll
    for (int d = 0; d < kWords<N>; ++d) q[d] = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) bits_put(q, 6 * j, 6, kern::mx_sr_e2m3(__float_as_uint(f[j] * sc.inv), word(j)));
    if (sc.blank) {
#pragma unroll
      for (int d = 0; d < kWords<N>; ++d) q[d] = 0u;
    }
  }
  template <int N> __device__ static __forceinline__ void unpack(const uint32_t* q, float scale, float* f) {
#pragma unroll
    for (int g = 0; g < N / 4; ++g) fp6_widen4(bits_get(q, 24 * g, 24), scale, f + 4 * g);
  }
  // `pay`: the chunk's payload, v: the lane's vector in the chunk (its low bits are the lane's place in
  // its quad / pair: spans start at multiples of 64). EPL = 4: lane i of a quad owns bits 24 i .. 24 i + 23
  // of the quad's 96 and moves dword i of its three (lane 3: none), at byte 12 (v / 4) + 4 i = 3 v + i.
  // EPL = 8: lane p of a pair owns bits 48 p .. 48 p + 47; lane 0 moves dwords 0 and 1, lane 1 dword 2.
  template <int EPL> __device__ static __forceinline__ void ld_lanes(const char* pay, uint32_t v, uint32_t* q) {
    if constexpr (EPL == 4) {
      const uint32_t i = v & 3u;
      q[0] = i < 3u ? *reinterpret_cast<const uint32_t*>(pay + 3 * (size_t)v + i) : 0u;
    } else {
      const uint32_t p = v & 1u;
      const char* at = pay + 12 * (size_t)(v >> 1);
      q[0] = *reinterpret_cast<const uint32_t*>(at + 8 * p);
      q[1] = p ? 0u : *reinterpret_cast<const uint32_t*>(at + 4);
    }
  }
  template <int EPL> __device__ static __forceinline__ void gather(uint32_t v, uint32_t* q) {
    if constexpr (EPL == 4) {
      const uint32_t i = v & 3u;
      const uint32_t prev = dpp_mov<kDppQuadPrev>(q[0]);  // dword i - 1 of the quad
      q[0] = (uint32_t)((((uint64_t)q[0] << 32) | prev) >> (32u - 8u * i));
    } else {
      const uint32_t mid = dpp_mov<kDppPairEven>(q[1]);  // dword 1 of the pair
      if (v & 1u) {
        const uint32_t d2 = q[0];
        q[0] = (mid >> 16) | (d2 << 16);
        q[1] = d2 >> 16;
      }
    }
  }
  template <int EPL> __device__ static __forceinline__ void st_lanes(char* pay, uint32_t v, const uint32_t* q) {
    if constexpr (EPL == 4) {
      const uint32_t i = v & 3u;
      const uint32_t next = dpp_mov<kDppQuadNext>(q[0]);  // the 24 bits of lane i + 1
      if (i < 3u) *reinterpret_cast<uint32_t*>(pay + 3 * (size_t)v + i) = (q[0] >> (8u * i)) | (next << (24u - 8u * i));
    } else {
      const uint32_t p = v & 1u;
      const uint32_t next = dpp_mov<kDppPairOdd>(q[0]);  // the low 32 bits of lane 1
      char* at = pay + 12 * (size_t)(v >> 1);
      *reinterpret_cast<uint32_t*>(at + 8 * p) = p ? (q[0] >> 16) | (q[1] << 16) : q[0];
      if (!p) *reinterpret_cast<uint32_t*>(at + 4) = (q[1] & 0xffffu) | (next << 16);
    }
  }
};

// The new residual of an element: v - d, +0 where that is not finite. d is the product of a payload value
// and a power of two: exact while it is finite, so a fused multiply-subtract gives the same bits
// there; where the product overflowed (the top of the f32 range) or is NaN (scale byte 255) the
// contract's v - d is not finite either, which the test on d itself catches whatever was fused.
__device__ __forceinline__ float ef_residual(float v, float d) {
  const float r = v - d;
  return abs_bits(d) < 0x7f800000u && abs_bits(r) < 0x7f800000u ? r : 0.0f;
}

// The random words of a lane's consecutive elements (mx_sr.h): element j has the index i0 + j. The
// indices of one lane may straddle a multiple of 2^32, where the key changes; both keys are the call's
// key itself while the index base and the tensor stay below 2^32.
struct SrWords {
  uint32_t lo, kh0, kh1;
  __device__ __forceinline__ SrWords(uint32_t key, uint64_t i0, int n) {
    lo = (uint32_t)i0;
    const uint32_t h = (uint32_t)(i0 >> 32);
    kh0 = kern::mx_sr_key_h(key, h);
    kh1 = kh0;
    if (lo + (uint32_t)(n - 1) < lo) kh1 = kern::mx_sr_key_h(key, h + 1u);
  }
  __device__ __forceinline__ uint32_t operator()(int j) const {
    const uint32_t l = lo + (uint32_t)j;
    return kern::mx_sr_word_lo(l < lo ? kh1 : kh0, l);
  }
};
// ... and of a chunk's own elements (reduce): 32 cb <= 2^32 of them, so the key is the call's
struct SrChunkWords {
  uint32_t lo, key;
  __device__ __forceinline__ uint32_t operator()(int j) const { return kern::mx_sr_word_lo(key, lo + (uint32_t)j); }
};

// B (2, 4, 8 or 16) wire bytes at p (B-aligned) <-> the low bytes of q[(B + 3) / 4]; B = 24: p is 8-byte
// aligned and the bytes move as three 8-byte accesses
template <int B>
__device__ __forceinline__ void ld_wire(const char* p, uint32_t* q) {
  if constexpr (B == 2) {
    q[0] = *reinterpret_cast<const uint16_t*>(p);
  } else if constexpr (B == 4) {
    q[0] = *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (B == 8) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    q[0] = x.x;
    q[1] = x.y;
  } else if constexpr (B == 24) {
    ld_wire<8>(p, q);
    ld_wire<8>(p + 8, q + 2);
    ld_wire<8>(p + 16, q + 4);
  } else {
    const uint4 x = *reinterpret_cast<const uint4*>(p);
    q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w;
  }
}
template <int B>
__device__ __forceinline__ void st_wire(char* p, const uint32_t* q) {
  if constexpr (B == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)q[0];
  else if constexpr (B == 4) *reinterpret_cast<uint32_t*>(p) = q[0];
  else if constexpr (B == 8) *reinterpret_cast<uint2*>(p) = make_uint2(q[0], q[1]);
  else if constexpr (B == 24) {
    st_wire<8>(p, q);
    st_wire<8>(p + 8, q + 2);
    st_wire<8>(p + 16, q + 4);
  } else *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
}

// ---------------------------------------------------------------------------- quantize
// Lane layout of one chunk (grid row): vector v of the chunk is 16 B of the tensor = EPL elements,
// LPB = 32 / EPL consecutive lanes make a block. The chunk has cb * LPB vectors, a multiple of 64.
// SHARD: chunk r is the `m` elements from r * m on (numel = nchunks * m) instead of the 32 cb from
// r * 32 cb on, and nothing at or past (r + 1) * m enters it. VEC = false (shards that do not start
// 16-byte aligned) reads every element on its own. On the wire a lane stores QB = EPL (FP8) or
// EPL / 2 (FP4) payload bytes; FP6: 3 EPL / 4 bytes, as the aligned dwords of MxFmt's st_lanes.
//
// EF (error feedback, docs/collectives.md "Error feedback"): what is quantized is v = x + res, and res
// becomes v - D(Q(v)) where that is finite, +0 where it is not. `res` holds one float per element of
// the tensor, at the element's own index, so a lane's EPL floats are one or two 16-B vectors that
// are aligned whenever its 16 B of the tensor are; nothing at or past the chunk's end is read or
// written. The dequantized values come from the lane's own packed dwords.
//
// SR (stochastic rounding, never together with EF): the payload is rounded up or down by the word of
// the element's index, `sr_base` plus its index in the tensor -- the same in the dealt and the shard
// layout. The lane computes its EPL words itself; the scale byte and everything else are unchanged.
//
// ROT (docs/collectives.md "Hadamard rotation"): every block is rotated (rot_forward) right after it is
// widened, padding zeros included, so the residual is added to and taken from the rotated block.
// `rot_signs` is the call's sign word.
template <MxFormat F, DType DT, bool SHARD, bool VEC, bool EF, bool SR, bool ROT>
__global__ __launch_bounds__(256) void k_mx_quantize(const char* __restrict__ src, size_t numel,
                                                     char* __restrict__ wire, uint32_t cb, size_t m,
                                                     float* __restrict__ res, uint32_t sr_key, uint64_t sr_base,
                                                     uint32_t rot_signs) {
  static_assert(!(EF && SR), "error feedback and stochastic rounding are alternatives");
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  using M = MxFmt<F>;
  constexpr int QB = EPL * M::kPayload / kern::kMxBlock, QW = M::template kWords<EPL>;
  const size_t chunk = blockIdx.y;
  char* __restrict__ w = wire + chunk * kern::mx_chunk_bytes(F, cb);
  const size_t el0 = SHARD ? chunk * m : chunk * cb * (size_t)kern::kMxBlock;  // first element of the chunk
  const size_t end = SHARD ? el0 + m : numel;                                  // one past its last
  const uint32_t nvec = cb * LPB;
  // a workgroup takes one contiguous span of kMxUnroll * 256 vectors per pass (16 KiB of the tensor)
  constexpr uint32_t stride = 256u;
  const uint32_t pass = gridDim.x * 256u * kMxUnroll;
  for (uint32_t v0 = blockIdx.x * 256u * kMxUnroll + threadIdx.x; v0 < nvec; v0 += pass) {
    S s[kMxUnroll][EPL];
    float r[EF ? kMxUnroll : 1][EPL];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      const size_t el = el0 + (size_t)v * EPL;
      if (VEC && v < nvec && el + EPL <= end) {
        const uint4 x = *reinterpret_cast<const uint4*>(src + el * sizeof(S));
        __builtin_memcpy(s[u], &x, 16);
        if constexpr (EF) {
#pragma unroll
          for (int j = 0; j < EPL / 4; ++j) {
            const uint4 y = *reinterpret_cast<const uint4*>(res + el + 4 * j);
            __builtin_memcpy(&r[u][4 * j], &y, 16);
          }
        }
      } else {
        // the last vector, or padding: elements past the end count as +0 and are never read
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
          S z;
          __builtin_memset(&z, 0, sizeof(S));
          if (v < nvec && el + i < end) z = reinterpret_cast<const S*>(src)[el + i];
          s[u][i] = z;
          if constexpr (EF) r[u][i] = v < nvec && el + i < end ? res[el + i] : 0.0f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      if (v >= nvec) break;  // (whole waves leave together: nvec and every span start are multiples of 64)
      float f[EPL];
      uint32_t am = 0;
      if constexpr (ROT) {  // (whole blocks are here: nvec is a multiple of LPB)
#pragma unroll
        for (int i = 0; i < EPL; ++i) f[i] = T::in(s[u][i]);
        rot_forward<EPL>(f, rot_signs, v % LPB);
      }
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        if constexpr (!ROT) f[i] = T::in(s[u][i]);
        if constexpr (EF) f[i] += r[u][i];
        const uint32_t a = abs_bits(f[i]);
        am = a > am ? a : am;
      }
      const MxScale sc = M::scale(group_max<LPB>(am));
      uint32_t q[QW];
      if constexpr (SR) M::template pack_sr<EPL>(f, sc, q, SrWords(sr_key, sr_base + el0 + (uint64_t)v * EPL, EPL));
      else M::template pack<EPL>(f, sc, q);
      // FP8: payload byte e of the chunk is element e of the chunk; FP4: byte e holds elements 2e, 2e + 1
      if constexpr (M::kLanes) M::template st_lanes<EPL>(w, v, q);
      else st_wire<QB>(w + (size_t)v * QB, q);
      if (v % LPB == 0) w[kern::mx_scale_off(F, cb, v / LPB)] = (char)sc.byte;
      if constexpr (EF) {
        float d[EPL];
        M::template unpack<EPL>(q, mx_scale_value(sc.byte), d);
#pragma unroll
        for (int i = 0; i < EPL; ++i) d[i] = ef_residual(f[i], d[i]);
        const size_t el = el0 + (size_t)v * EPL;
        if (VEC && el + EPL <= end) {
#pragma unroll
          for (int j = 0; j < EPL / 4; ++j) {
            uint4 y;
            __builtin_memcpy(&y, &d[4 * j], 16);
            *reinterpret_cast<uint4*>(res + el + 4 * j) = y;
          }
        } else {
#pragma unroll
          for (int i = 0; i < EPL; ++i)
            if (el + i < end) res[el + i] = d[i];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------- dequantize
// The same lane layout as quantize: a lane reads EPL payload bytes and its block's scale byte and
// stores 16 B of the tensor; nothing at or past `numel` is written. SHARD / VEC as in quantize:
// chunk r fills exactly dst[r m, (r + 1) m).
//
// ROT: the block is rotated back (rot_inverse) before the cast. Its lanes exchange values, so the lanes of
// a partial last block all load, convert and take part -- the vectors are counted in whole blocks -- and
// only the stores are masked.
template <MxFormat F, DType DT, bool SHARD, bool VEC, bool ROT>
__global__ __launch_bounds__(256) void k_mx_dequantize(const char* __restrict__ wire, uint32_t cb,
                                                       char* __restrict__ dst, size_t numel, size_t m,
                                                       uint32_t rot_signs) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  using M = MxFmt<F>;
  constexpr int QB = EPL * M::kPayload / kern::kMxBlock, QW = M::template kWords<EPL>;
  const size_t chunk = blockIdx.y;
  const char* __restrict__ w = wire + chunk * kern::mx_chunk_bytes(F, cb);
  const size_t el0 = SHARD ? chunk * m : chunk * cb * (size_t)kern::kMxBlock;
  if (el0 >= numel) return;  // a padding chunk
  const size_t left = SHARD ? m : numel - el0;
  // vectors of this chunk that hold at least one element of the tensor
  uint32_t nvec = (uint32_t)(left >= (size_t)cb * kern::kMxBlock ? (size_t)cb * LPB : (left + EPL - 1) / EPL);
  if constexpr (ROT) nvec = (nvec + LPB - 1) / LPB * LPB;  // (<= cb * LPB, itself a multiple of LPB)
  constexpr uint32_t stride = 256u;  // (contiguous spans per workgroup, as in quantize)
  const uint32_t pass = gridDim.x * 256u * kMxUnroll;
  for (uint32_t v0 = blockIdx.x * 256u * kMxUnroll + threadIdx.x; v0 < nvec; v0 += pass) {
    uint32_t q[kMxUnroll][QW];
    uint32_t sb[kMxUnroll];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      sb[u] = 127u;
#pragma unroll
      for (int d = 0; d < QW; ++d) q[u][d] = 0u;
      if (v < nvec) {
        if constexpr (M::kLanes) M::template ld_lanes<EPL>(w, v, q[u]);
        else ld_wire<QB>(w + (size_t)v * QB, q[u]);
        sb[u] = (uint8_t)w[kern::mx_scale_off(F, cb, v / LPB)];
      }
    }
    if constexpr (M::kLanes) {  // (a lane in range has every lower lane of its quad / pair in range with it)
      // v % 4 is the lane's place in its hardware quad only while every span and step is whole quads
      static_assert(stride % 4 == 0 && (256u * kMxUnroll) % 64 == 0, "gather takes the quad lane from v");
#pragma unroll
      for (int u = 0; u < kMxUnroll; ++u) M::template gather<EPL>(v0 + u * stride, q[u]);
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      if (v >= nvec) break;
      const float scale = mx_scale_value(sb[u]);
      float f[EPL];
      M::template unpack<EPL>(q[u], scale, f);
      if constexpr (ROT) rot_inverse<EPL>(f, rot_signs, v % LPB);
      S s[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i) s[i] = T::out(f[i]);
      const size_t el = (size_t)v * EPL;  // within the chunk
      S* o = reinterpret_cast<S*>(dst) + el0 + el;
      if (VEC && el + EPL <= left) {
        uint4 x;
        __builtin_memcpy(&x, s, 16);
        *reinterpret_cast<uint4*>(o) = x;
      } else {
#pragma unroll
        for (int i = 0; i < EPL; ++i)
          if (el + i < left) o[i] = s[i];
      }
    }
  }
}

// ---------------------------------------------------------------------------- reduce
// A lane takes PB = 16 payload bytes of every source (FP6: 24). FP8: that is half a block, so a block is
// two neighbouring lanes and the amax of the folded block is one exchange between them. FP4, FP6: PB
// payload bytes are a whole block (EPL = 32), so the lane holds its block's amax and there is no
// exchange; the price is 32 accumulators per lane instead of 16.
//
// EF: the owner residual (32 cb floats, one per element of the chunk) is added to the fold after the
// AVG division and before the scale is taken, and becomes acc - D(Q(acc)) (+0 where not finite). A
// lane's EPL floats are contiguous: they are loaded with the payloads and stored a payload dword's
// elements at a time, straight from that dword.
//
// SR (never together with EF): the fold is requantized with the words of its elements' indices in the
// chunk, v EPL + i.
template <MxFormat F, int NSRC, bool AVG, bool EF, bool SR>
__global__ __launch_bounds__(256) void k_mx_reduce(const char* __restrict__ in, uint32_t cb, int avg_div,
                                                   char* __restrict__ out, float* __restrict__ res, uint32_t sr_key) {
  static_assert(!(EF && SR), "error feedback and stochastic rounding are alternatives");
  using M = MxFmt<F>;
  constexpr int PB = M::kPayload == 24 ? 24 : 16, PW = PB / 4;  // payload bytes / dwords of a lane
  constexpr int EPL = PB * kern::kMxBlock / M::kPayload;        // 16 or 32
  constexpr int LPB = kern::kMxBlock / EPL;                     // 2 or 1
  const size_t cbytes = kern::mx_chunk_bytes(F, cb);
  const uint32_t nvec = cb * (uint32_t)LPB;
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nvec; v += stride) {
    uint32_t p[NSRC][PW];
    uint32_t sb[NSRC];
#pragma unroll
    for (int r = 0; r < NSRC; ++r) {
      const char* c = in + (size_t)r * cbytes;
      ld_wire<PB>(c + (size_t)v * PB, p[r]);
      sb[r] = (uint8_t)c[kern::mx_scale_off(F, cb, v / LPB)];
    }
    uint4 rr[EF ? EPL / 4 : 1];
    if constexpr (EF) {
#pragma unroll
      for (int j = 0; j < EPL / 4; ++j) rr[j] = *reinterpret_cast<const uint4*>(res + (size_t)v * EPL + 4 * j);
    }
    float acc[EPL];
#pragma unroll
    for (int r = 0; r < NSRC; ++r) {
      const float scale = mx_scale_value(sb[r]);
      float f[EPL];
      M::template unpack<EPL>(p[r], scale, f);
#pragma unroll
      for (int i = 0; i < EPL; ++i) acc[i] = r == 0 ? f[i] : acc[i] + f[i];  // rank order
    }
    if constexpr (AVG) {
#pragma unroll
      for (int i = 0; i < EPL; ++i) acc[i] = acc[i] / (float)avg_div;
    }
    if constexpr (EF) {
#pragma unroll
      for (int j = 0; j < EPL / 4; ++j) {
        acc[4 * j] += __uint_as_float(rr[j].x);
        acc[4 * j + 1] += __uint_as_float(rr[j].y);
        acc[4 * j + 2] += __uint_as_float(rr[j].z);
        acc[4 * j + 3] += __uint_as_float(rr[j].w);
      }
    }
    uint32_t am = 0;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const uint32_t a = abs_bits(acc[i]);
      am = a > am ? a : am;
    }
    const MxScale sc = M::scale(group_max<LPB>(am));
    uint32_t q[PW];
    if constexpr (SR) M::template pack_sr<EPL>(acc, sc, q, SrChunkWords{v * (uint32_t)EPL, sr_key});
    else M::template pack<EPL>(acc, sc, q);
    st_wire<PB>(out + (size_t)v * PB, q);
    if (v % LPB == 0) out[kern::mx_scale_off(F, cb, v / LPB)] = (char)sc.byte;
    if constexpr (EF) {
      // elements and payload dwords of one step: a dword's 4 or 8, or the 16 of three FP6 dwords
      constexpr int G = M::kLanes ? 16 : EPL / 4, GW = M::kLanes ? 3 : 1;
      const float scale = mx_scale_value(sc.byte);
#pragma unroll
      for (int w = 0; w < EPL / G; ++w) {
        float d[G];
        M::template unpack<G>(q + GW * w, scale, d);
#pragma unroll
        for (int i = 0; i < G; ++i) d[i] = ef_residual(acc[G * w + i], d[i]);
#pragma unroll
        for (int j = 0; j < G / 4; ++j) {
          uint4 y;
          __builtin_memcpy(&y, &d[4 * j], 16);
          *reinterpret_cast<uint4*>(res + (size_t)v * EPL + G * w + 4 * j) = y;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------- fold
// nsrc chunk wires -> a tensor: what mx_reduce then mx_dequantize would give without the wire in
// between (and without its requantization). The lane layout is dequantize's: the wide side is the
// output, 16 B = EPL elements per lane, so a lane reads EPL (FP4: EPL / 2) payload bytes and its block's scale byte
// of every source and a wave's store is contiguous. All NSRC * U loads are issued before the first
// convert; U keeps about eight of them in flight per lane whatever NSRC is.
template <int NSRC>
constexpr int kMxFoldUnroll = NSRC <= 2 ? 4 : (NSRC <= 4 ? 2 : 1);

//
// ROT: the sources are folded as they are (the rotation is linear) and the fold is rotated back after the
// AVG division and before the cast; whole blocks take part, as in dequantize.
template <MxFormat F, DType DT, int NSRC, bool AVG, bool ROT>
__global__ __launch_bounds__(256) void k_mx_fold(const char* __restrict__ in, uint32_t cb, int avg_div,
                                                 char* __restrict__ dst, size_t numel, uint32_t rot_signs) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  constexpr int U = kMxFoldUnroll<NSRC>;
  using M = MxFmt<F>;
  constexpr int QB = EPL * M::kPayload / kern::kMxBlock, QW = M::template kWords<EPL>;
  const size_t cbytes = kern::mx_chunk_bytes(F, cb);
  uint32_t nvec = (uint32_t)((numel + EPL - 1) / EPL);  // <= cb * LPB: numel <= 32 cb
  if constexpr (ROT) nvec = (nvec + LPB - 1) / LPB * LPB;
  const uint32_t pass = gridDim.x * 256u * U;
  for (uint32_t v0 = blockIdx.x * 256u * U + threadIdx.x; v0 < nvec; v0 += pass) {
    uint32_t q[U][NSRC][QW];
    uint32_t sb[U][NSRC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t v = v0 + u * 256u;
#pragma unroll
      for (int r = 0; r < NSRC; ++r) {
        sb[u][r] = 127u;
#pragma unroll
        for (int d = 0; d < QW; ++d) q[u][r][d] = 0u;
        if (v < nvec) {
          const char* c = in + (size_t)r * cbytes;
          if constexpr (M::kLanes) M::template ld_lanes<EPL>(c, v, q[u][r]);
          else ld_wire<QB>(c + (size_t)v * QB, q[u][r]);
          sb[u][r] = (uint8_t)c[kern::mx_scale_off(F, cb, v / LPB)];
        }
      }
    }
    if constexpr (M::kLanes) {  // (as in dequantize: 256 lanes a step, whole quads)
      static_assert((256u * U) % 64 == 0, "gather takes the quad lane from v");
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < NSRC; ++r) M::template gather<EPL>(v0 + u * 256u, q[u][r]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t v = v0 + u * 256u;
      if (v >= nvec) break;
      float acc[EPL];
#pragma unroll
      for (int r = 0; r < NSRC; ++r) {
        const float scale = mx_scale_value(sb[u][r]);
        float f[EPL];
        M::template unpack<EPL>(q[u][r], scale, f);
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = r == 0 ? f[i] : acc[i] + f[i];  // source order
      }
      if constexpr (AVG) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = acc[i] / (float)avg_div;
      }
      if constexpr (ROT) rot_inverse<EPL>(acc, rot_signs, v % LPB);
      S s[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i) s[i] = T::out(acc[i]);
      const size_t el = (size_t)v * EPL;
      S* o = reinterpret_cast<S*>(dst) + el;
      if (el + EPL <= numel) {
        uint4 x;
        __builtin_memcpy(&x, s, 16);
        *reinterpret_cast<uint4*>(o) = x;
      } else {
#pragma unroll
        for (int i = 0; i < EPL; ++i)
          if (el + i < numel) o[i] = s[i];
      }
    }
  }
}

// grid row of `nvec` vectors with `per` of them per lane and pass, at most `most` workgroups in all
// rows (the kernels loop past that). Quantize / dequantize: one pass per workgroup up to 2^20 of them;
// reduce: a grid-stride loop over 8 workgroups per CU.
constexpr uint64_t kMxGridStream = uint64_t(1) << 20, kMxGridReduce = 2048;
inline uint32_t mx_grid_x(uint64_t nvec, int per, size_t rows, uint64_t most) {
  const uint64_t want = (nvec + 256u * per - 1) / (256u * per);
  const uint64_t cap = std::max<uint64_t>(1, most / std::max<size_t>(1, rows));
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

}  // namespace
}  // namespace dev

namespace kern {

namespace {
bool mx_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// cb: a multiple of 16, and a chunk's lanes are counted in 32 bits
bool mx_cb_ok(size_t cb) { return cb > 0 && cb % kMxScaleAlign == 0 && cb <= (size_t(1) << 27); }
bool mx_fmt_ok(MxFormat f) { return f == MxFormat::FP8_E4M3 || f == MxFormat::FP4_E2M1 || f == MxFormat::FP6_E2M3; }
size_t mx_esize(DType t) { return t == DType::F32 ? 4 : 2; }
bool mx_dtype_ok(DType t) { return t == DType::F32 || t == DType::BF16 || t == DType::F16; }
// the shard arguments: m elements per shard fit the chunk, and the whole tensor's size is a size_t
bool mx_shards_ok(size_t m, size_t cb, size_t nchunks) {
  return mx_cb_ok(cb) && m > 0 && m <= cb * kMxBlock && nchunks > 0 && nchunks <= 65535;
}
dim3 mx_stream_grid(size_t cb, DType t, size_t nchunks) {
  const int lpb = t == DType::F32 ? 8 : 4;
  return dim3(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
}

// key and index base of a stochastic call (mx_sr.h); null: round to nearest
struct MxSr {
  uint32_t key;
  uint64_t base;
};
// quantize / dequantize of one format and dtype: the dealt kernel, or the shard one with or without vectors
template <MxFormat F, DType DT, bool EF, bool SR, bool ROT>
void mx_quantize_ef_go(bool shard, bool vec, const dim3& grid, const char* s, size_t numel, char* w, uint32_t cb,
                       size_t m, float* res, uint32_t key, uint64_t base, uint32_t signs, hipStream_t stream) {
  if (!shard) hipLaunchKernelGGL((dev::k_mx_quantize<F, DT, false, true, EF, SR, ROT>), grid, dim3(256), 0, stream, s, numel, w, cb, m, res, key, base, signs);
  else if (vec) hipLaunchKernelGGL((dev::k_mx_quantize<F, DT, true, true, EF, SR, ROT>), grid, dim3(256), 0, stream, s, numel, w, cb, m, res, key, base, signs);
  else hipLaunchKernelGGL((dev::k_mx_quantize<F, DT, true, false, EF, SR, ROT>), grid, dim3(256), 0, stream, s, numel, w, cb, m, res, key, base, signs);
}
// (`sr`: the stochastic kernels; else `res` null: the plain kernels; otherwise the error-feedback ones)
template <MxFormat F, DType DT, bool ROT>
void mx_quantize_rot_go(bool shard, bool vec, const dim3& grid, const char* s, size_t numel, char* w, uint32_t cb, size_t m,
                        float* res, const MxSr* sr, uint32_t signs, hipStream_t stream) {
  if (sr) mx_quantize_ef_go<F, DT, false, true, ROT>(shard, vec, grid, s, numel, w, cb, m, nullptr, sr->key, sr->base, signs, stream);
  else if (res) mx_quantize_ef_go<F, DT, true, false, ROT>(shard, vec, grid, s, numel, w, cb, m, res, 0u, 0u, signs, stream);
  else mx_quantize_ef_go<F, DT, false, false, ROT>(shard, vec, grid, s, numel, w, cb, m, res, 0u, 0u, signs, stream);
}
// (`rot`: the sign word of the rotated kernels; null: the kernels without the rotation)
template <MxFormat F, DType DT>
void mx_quantize_go(bool shard, bool vec, const dim3& grid, const char* s, size_t numel, char* w, uint32_t cb, size_t m,
                    float* res, const MxSr* sr, const uint32_t* rot, hipStream_t stream) {
  if (rot) mx_quantize_rot_go<F, DT, true>(shard, vec, grid, s, numel, w, cb, m, res, sr, *rot, stream);
  else mx_quantize_rot_go<F, DT, false>(shard, vec, grid, s, numel, w, cb, m, res, sr, 0u, stream);
}
template <MxFormat F, DType DT, bool ROT>
void mx_dequantize_rot_go(bool shard, bool vec, const dim3& grid, const char* w, uint32_t cb, char* d, size_t numel, size_t m,
                          uint32_t signs, hipStream_t stream) {
  if (!shard) hipLaunchKernelGGL((dev::k_mx_dequantize<F, DT, false, true, ROT>), grid, dim3(256), 0, stream, w, cb, d, numel, m, signs);
  else if (vec) hipLaunchKernelGGL((dev::k_mx_dequantize<F, DT, true, true, ROT>), grid, dim3(256), 0, stream, w, cb, d, numel, m, signs);
  else hipLaunchKernelGGL((dev::k_mx_dequantize<F, DT, true, false, ROT>), grid, dim3(256), 0, stream, w, cb, d, numel, m, signs);
}
template <MxFormat F, DType DT>
void mx_dequantize_go(bool shard, bool vec, const dim3& grid, const char* w, uint32_t cb, char* d, size_t numel, size_t m,
                      const uint32_t* rot, hipStream_t stream) {
  if (rot) mx_dequantize_rot_go<F, DT, true>(shard, vec, grid, w, cb, d, numel, m, *rot, stream);
  else mx_dequantize_rot_go<F, DT, false>(shard, vec, grid, w, cb, d, numel, m, 0u, stream);
}
template <MxFormat F, class... A>
void mx_quantize_dt(DType t, A... a) {
  switch (t) {
    case DType::F32: mx_quantize_go<F, DType::F32>(a...); break;
    case DType::BF16: mx_quantize_go<F, DType::BF16>(a...); break;
    default: mx_quantize_go<F, DType::F16>(a...); break;
  }
}
template <MxFormat F, class... A>
void mx_dequantize_dt(DType t, A... a) {
  switch (t) {
    case DType::F32: mx_dequantize_go<F, DType::F32>(a...); break;
    case DType::BF16: mx_dequantize_go<F, DType::BF16>(a...); break;
    default: mx_dequantize_go<F, DType::F16>(a...); break;
  }
}
hipError_t mx_quantize_any(MxFormat fmt, DType t, bool shard, bool vec, const void* src, size_t numel, void* wire,
                           size_t cb, size_t nchunks, size_t m, hipStream_t stream, const uint32_t* rot,
                           float* res = nullptr, const MxSr* sr = nullptr) {
  const dim3 grid = mx_stream_grid(cb, t, nchunks);
  const char* s = static_cast<const char*>(src);
  char* w = static_cast<char*>(wire);
  if (fmt == MxFormat::FP4_E2M1) mx_quantize_dt<MxFormat::FP4_E2M1>(t, shard, vec, grid, s, numel, w, (uint32_t)cb, m, res, sr, rot, stream);
  else if (fmt == MxFormat::FP6_E2M3) mx_quantize_dt<MxFormat::FP6_E2M3>(t, shard, vec, grid, s, numel, w, (uint32_t)cb, m, res, sr, rot, stream);
  else mx_quantize_dt<MxFormat::FP8_E4M3>(t, shard, vec, grid, s, numel, w, (uint32_t)cb, m, res, sr, rot, stream);
  return hipGetLastError();
}
hipError_t mx_dequantize_any(MxFormat fmt, DType t, bool shard, bool vec, const void* wire, size_t cb, size_t nchunks,
                             void* dst, size_t numel, size_t m, hipStream_t stream, const uint32_t* rot) {
  const dim3 grid = mx_stream_grid(cb, t, nchunks);
  const char* w = static_cast<const char*>(wire);
  char* d = static_cast<char*>(dst);
  if (fmt == MxFormat::FP4_E2M1) mx_dequantize_dt<MxFormat::FP4_E2M1>(t, shard, vec, grid, w, (uint32_t)cb, d, numel, m, rot, stream);
  else if (fmt == MxFormat::FP6_E2M3) mx_dequantize_dt<MxFormat::FP6_E2M3>(t, shard, vec, grid, w, (uint32_t)cb, d, numel, m, rot, stream);
  else mx_dequantize_dt<MxFormat::FP8_E4M3>(t, shard, vec, grid, w, (uint32_t)cb, d, numel, m, rot, stream);
  return hipGetLastError();
}
}  // namespace

hipError_t mx_quantize(const void* src, size_t numel, DType t, void* wire, size_t cb, size_t nchunks,
                       hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(src)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock) return hipErrorInvalidValue;
  return mx_quantize_any(fmt, t, false, true, src, numel, wire, cb, nchunks, 0, stream, rot_signs);
}

hipError_t mx_dequantize(const void* wire, size_t cb, size_t nchunks, void* dst, size_t numel, DType t,
                         hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(dst)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  return mx_dequantize_any(fmt, t, false, true, wire, cb, nchunks, dst, numel, 0, stream, rot_signs);
}

hipError_t mx_quantize_shards(const void* src, size_t m, DType t, void* wire, size_t cb, size_t nchunks,
                              hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(src)) return hipErrorInvalidValue;
  const bool vec = m * mx_esize(t) % 16 == 0;  // every shard starts 16-byte aligned
  return mx_quantize_any(fmt, t, true, vec, src, m * nchunks, wire, cb, nchunks, m, stream, rot_signs);
}

hipError_t mx_quantize_ef(const void* src, size_t numel, DType t, float* residual, void* wire, size_t cb,
                          size_t nchunks, hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(src)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock || (numel && (!residual || !mx_al16(residual)))) return hipErrorInvalidValue;
  // (no elements: no residual to update, the wire is all padding blocks)
  return mx_quantize_any(fmt, t, false, true, src, numel, wire, cb, nchunks, 0, stream, rot_signs, numel ? residual : nullptr);
}

hipError_t mx_quantize_shards_ef(const void* src, size_t m, DType t, float* residual, void* wire, size_t cb,
                                 size_t nchunks, hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(src) || !residual || !mx_al16(residual))
    return hipErrorInvalidValue;
  const bool vec = m * mx_esize(t) % 16 == 0;  // every shard, and its slice of the residual, starts 16-byte aligned
  return mx_quantize_any(fmt, t, true, vec, src, m * nchunks, wire, cb, nchunks, m, stream, rot_signs, residual);
}

hipError_t mx_quantize_sr(const void* src, size_t numel, DType t, void* wire, size_t cb, size_t nchunks,
                          uint64_t seed, uint32_t sr_stream, uint64_t index_offset, hipStream_t stream, MxFormat fmt,
                          const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(src)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock || index_offset + numel < index_offset) return hipErrorInvalidValue;
  const MxSr sr{mx_sr_key(seed, sr_stream), index_offset};
  return mx_quantize_any(fmt, t, false, true, src, numel, wire, cb, nchunks, 0, stream, rot_signs, nullptr, &sr);
}

hipError_t mx_quantize_shards_sr(const void* src, size_t m, DType t, void* wire, size_t cb, size_t nchunks,
                                 uint64_t seed, uint32_t sr_stream, uint64_t index_offset, hipStream_t stream,
                                 MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(src)) return hipErrorInvalidValue;
  if (index_offset + m * nchunks < index_offset) return hipErrorInvalidValue;
  const bool vec = m * mx_esize(t) % 16 == 0;
  const MxSr sr{mx_sr_key(seed, sr_stream), index_offset};
  return mx_quantize_any(fmt, t, true, vec, src, m * nchunks, wire, cb, nchunks, m, stream, rot_signs, nullptr, &sr);
}

hipError_t mx_dequantize_shards(const void* wire, size_t cb, size_t nchunks, void* dst, size_t m, DType t,
                                hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_dtype_ok(t)) return hipErrorInvalidValue;
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(dst)) return hipErrorInvalidValue;
  const bool vec = m * mx_esize(t) % 16 == 0;
  return mx_dequantize_any(fmt, t, true, vec, wire, cb, nchunks, dst, m * nchunks, m, stream, rot_signs);
}

namespace {
template <MxFormat F, bool AVG, bool EF, bool SR>
hipError_t mx_reduce_go(const char* in, int nsrc, uint32_t cb, int avg_div, char* out, float* res, uint32_t key,
                        hipStream_t stream) {
  constexpr int lpb = F == MxFormat::FP8_E4M3 ? 2 : 1;  // lanes per block: 16 (FP6: 24) payload bytes per lane
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, 1, 1, dev::kMxGridReduce)), block(256);
  switch (nsrc) {
#define PDCC_MX_N(N) \
  case N: hipLaunchKernelGGL((dev::k_mx_reduce<F, N, AVG, EF, SR>), grid, block, 0, stream, in, cb, avg_div, out, res, key); break;
    PDCC_MX_N(1) PDCC_MX_N(2) PDCC_MX_N(3) PDCC_MX_N(4) PDCC_MX_N(5) PDCC_MX_N(6) PDCC_MX_N(7) PDCC_MX_N(8)
#undef PDCC_MX_N
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// (`key`: the stochastic kernels; else `res` null: the plain kernels; otherwise the error-feedback ones)
template <MxFormat F>
hipError_t mx_reduce_op(const char* in, int nsrc, uint32_t cb, RedOp op, int avg_div, char* out, float* res,
                        const uint32_t* key, hipStream_t stream) {
  if (key)
    return op == RedOp::AVG ? mx_reduce_go<F, true, false, true>(in, nsrc, cb, avg_div, out, nullptr, *key, stream)
                            : mx_reduce_go<F, false, false, true>(in, nsrc, cb, avg_div, out, nullptr, *key, stream);
  if (res)
    return op == RedOp::AVG ? mx_reduce_go<F, true, true, false>(in, nsrc, cb, avg_div, out, res, 0u, stream)
                            : mx_reduce_go<F, false, true, false>(in, nsrc, cb, avg_div, out, res, 0u, stream);
  return op == RedOp::AVG ? mx_reduce_go<F, true, false, false>(in, nsrc, cb, avg_div, out, res, 0u, stream)
                          : mx_reduce_go<F, false, false, false>(in, nsrc, cb, avg_div, out, res, 0u, stream);
}
hipError_t mx_reduce_any(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out, float* res,
                         hipStream_t stream, MxFormat fmt, const uint32_t* key = nullptr) {
  if (!mx_fmt_ok(fmt) || !mx_cb_ok(cb) || nsrc < 1 || nsrc > kMaxRanks || !mx_al16(wire_in) || !mx_al16(wire_out))
    return hipErrorInvalidValue;
  if (op != RedOp::SUM && op != RedOp::AVG) return hipErrorInvalidValue;
  if (op == RedOp::AVG && avg_div < 1) return hipErrorInvalidValue;
  const char* in = static_cast<const char*>(wire_in);
  char* out = static_cast<char*>(wire_out);
  if (fmt == MxFormat::FP6_E2M3) return mx_reduce_op<MxFormat::FP6_E2M3>(in, nsrc, (uint32_t)cb, op, avg_div, out, res, key, stream);
  return fmt == MxFormat::FP4_E2M1 ? mx_reduce_op<MxFormat::FP4_E2M1>(in, nsrc, (uint32_t)cb, op, avg_div, out, res, key, stream)
                                   : mx_reduce_op<MxFormat::FP8_E4M3>(in, nsrc, (uint32_t)cb, op, avg_div, out, res, key, stream);
}
}  // namespace

hipError_t mx_reduce(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out,
                     hipStream_t stream, MxFormat fmt) {
  return mx_reduce_any(wire_in, nsrc, cb, op, avg_div, wire_out, nullptr, stream, fmt);
}

hipError_t mx_reduce_ef(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, float* residual,
                        void* wire_out, hipStream_t stream, MxFormat fmt) {
  if (!residual || !mx_al16(residual)) return hipErrorInvalidValue;
  return mx_reduce_any(wire_in, nsrc, cb, op, avg_div, wire_out, residual, stream, fmt);
}

hipError_t mx_reduce_sr(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out, uint64_t seed,
                        uint32_t sr_stream, hipStream_t stream, MxFormat fmt) {
  const uint32_t key = mx_sr_key(seed, sr_stream);
  return mx_reduce_any(wire_in, nsrc, cb, op, avg_div, wire_out, nullptr, stream, fmt, &key);
}

namespace {
template <MxFormat F, DType DT, bool AVG, bool ROT>
hipError_t mx_fold_go(const char* in, int nsrc, uint32_t cb, int avg_div, char* dst, size_t numel, uint32_t signs,
                      hipStream_t stream) {
  constexpr int epl = 16 / (int)sizeof(typename dev::Tr<DT>::S);
  const uint64_t nvec = (numel + epl - 1) / epl;
  const dim3 block(256);
  switch (nsrc) {
#define PDCC_MX_N(N)                                                                                                       \
  case N: {                                                                                                                \
    const dim3 grid(dev::mx_grid_x(nvec, dev::kMxFoldUnroll<N>, 1, dev::kMxGridReduce));                                   \
    hipLaunchKernelGGL((dev::k_mx_fold<F, DT, N, AVG, ROT>), grid, block, 0, stream, in, cb, avg_div, dst, numel, signs); \
    break;                                                                                                                 \
  }
    PDCC_MX_N(1) PDCC_MX_N(2) PDCC_MX_N(3) PDCC_MX_N(4) PDCC_MX_N(5) PDCC_MX_N(6) PDCC_MX_N(7) PDCC_MX_N(8)
#undef PDCC_MX_N
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <MxFormat F, DType DT>
hipError_t mx_fold_op(const char* in, int nsrc, uint32_t cb, RedOp op, int avg_div, char* dst, size_t numel,
                      const uint32_t* rot, hipStream_t stream) {
  if (rot)
    return op == RedOp::AVG ? mx_fold_go<F, DT, true, true>(in, nsrc, cb, avg_div, dst, numel, *rot, stream)
                            : mx_fold_go<F, DT, false, true>(in, nsrc, cb, avg_div, dst, numel, *rot, stream);
  return op == RedOp::AVG ? mx_fold_go<F, DT, true, false>(in, nsrc, cb, avg_div, dst, numel, 0u, stream)
                          : mx_fold_go<F, DT, false, false>(in, nsrc, cb, avg_div, dst, numel, 0u, stream);
}
template <MxFormat F>
hipError_t mx_fold_dt(DType t, const char* in, int nsrc, uint32_t cb, RedOp op, int avg_div, char* d, size_t numel,
                      const uint32_t* rot, hipStream_t stream) {
  switch (t) {
    case DType::F32: return mx_fold_op<F, DType::F32>(in, nsrc, cb, op, avg_div, d, numel, rot, stream);
    case DType::BF16: return mx_fold_op<F, DType::BF16>(in, nsrc, cb, op, avg_div, d, numel, rot, stream);
    case DType::F16: return mx_fold_op<F, DType::F16>(in, nsrc, cb, op, avg_div, d, numel, rot, stream);
    default: return hipErrorInvalidValue;
  }
}
}  // namespace

hipError_t mx_fold(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* dst, size_t numel, DType t,
                   hipStream_t stream, MxFormat fmt, const uint32_t* rot_signs) {
  if (!mx_fmt_ok(fmt) || !mx_cb_ok(cb) || nsrc < 1 || nsrc > kMaxRanks || !mx_al16(wire_in) || !mx_al16(dst))
    return hipErrorInvalidValue;
  if (numel == 0 || numel > cb * kMxBlock) return hipErrorInvalidValue;
  if (op != RedOp::SUM && op != RedOp::AVG) return hipErrorInvalidValue;
  if (op == RedOp::AVG && avg_div < 1) return hipErrorInvalidValue;
  const char* in = static_cast<const char*>(wire_in);
  char* d = static_cast<char*>(dst);
  if (fmt == MxFormat::FP6_E2M3) return mx_fold_dt<MxFormat::FP6_E2M3>(t, in, nsrc, (uint32_t)cb, op, avg_div, d, numel, rot_signs, stream);
  return fmt == MxFormat::FP4_E2M1 ? mx_fold_dt<MxFormat::FP4_E2M1>(t, in, nsrc, (uint32_t)cb, op, avg_div, d, numel, rot_signs, stream)
                                   : mx_fold_dt<MxFormat::FP8_E4M3>(t, in, nsrc, (uint32_t)cb, op, avg_div, d, numel, rot_signs, stream);
}

}  // namespace kern
}  // namespace pdcc
