// What a kernel needs of one block-scaled wire format (mx_layout.h) beyond the block itself (mx_block.h): the scale
// rule, N elements to and from their payload bits, and the accesses of the payload on the wire. mx_wire.hip (the wire
// kernels) and adamw.hip / adamw8.hip (the fused AdamW step that emits the parameter wire) read this one definition.
// Contract: docs/collectives.md "Compressed all-reduce", "The `mxfp4_e2m1` wire format", "The `mxfp6_e2m3` wire format".
#pragma once
#include "dev_common.h"
#include "mx_block.h"
#include "mx_layout.h"
#include "mx_sr.h"

namespace pdcc {
namespace dev {

// e2m1: element 2j of a dword's eight sits in the low nibble of byte j, element 2j + 1 in the high one.
// The scale operand of the converts is 1: the kernels multiply in f32 (see the top of mx_wire.hip).
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
template <kern::MxFormat F> struct MxFmt;
template <> struct MxFmt<kern::MxFormat::FP8_E4M3> {
  static constexpr int kPayload = 32;
  static constexpr bool kLanes = false;
  template <int N> static constexpr int kWords = N / 4;
  // the largest magnitude is 448 = 1.75 2^8: e = k - 8 for m <= 1.75 and k - 7 above
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx_scale_of<8, 0x600000u, -117, 120>(amax); }
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
template <> struct MxFmt<kern::MxFormat::FP4_E2M1> {
  static constexpr int kPayload = 16;
  static constexpr bool kLanes = false;
  template <int N> static constexpr int kWords = (N + 7) / 8;
  // the largest magnitude is 6 = 1.5 2^2: e = k - 2 for m <= 1.5 and k - 1 above; the lower clamp keeps
  // 0.5 2^e a normal f32, the upper one is never reached (k <= 127)
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx_scale_of<2, 0x400000u, -125, 126>(amax); }
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
template <> struct MxFmt<kern::MxFormat::FP6_E2M3> {
  static constexpr int kPayload = 24;
  static constexpr bool kLanes = true;
  template <int N> static constexpr int kWords = (6 * N + 31) / 32;  // 4: 24 bits, 8: 48, 16: 96, 32: 192
  // the largest magnitude is 7.5 = 1.875 2^2: e = k - 2 for m <= 1.875 and k - 1 above; the lower clamp
  // keeps 0.125 2^e a normal f32, the upper one is never reached (k <= 127)
  __device__ static __forceinline__ MxScale scale(uint32_t amax) { return mx_scale_of<2, 0x700000u, -123, 126>(amax); }
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

// ---- the fused AdamW step's wire (adamw.hip, adamw8.hip; docs/collectives.md "Parameter wire from the step").
// kNoWire in place of an MxFormat: the instantiations that emit nothing.
constexpr int kNoWire = -1;

// Group `gi` of a one-chunk wire of `cb` blocks, as the f32 k_mx_quantize (EPL = 4, LPB = 8) writes it: the
// four values f of elements 4 gi .. 4 gi + 3 -> their payload bits and, from the block's first lane, the scale byte.
// The eight lanes of block gi / 8 are adjacent in the wave and all active (so are the four of a quad: the FP6 trade).
template <kern::MxFormat F>
__device__ __forceinline__ void mx_emit4(char* w, size_t cb, size_t gi, const float* f) {
  using M = MxFmt<F>;
  constexpr int QB = 4 * M::kPayload / kern::kMxBlock;  // payload bytes of the group: 4, 2 or (as bits) 3
  uint32_t am = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t a = abs_bits(f[j]);
    am = a > am ? a : am;
  }
  const MxScale sc = M::scale(group_max<8>(am));
  uint32_t q[1];
  M::template pack<4>(f, sc, q);
  // st_lanes finds its dword at 3 v + (v & 3): the quad's 12 bytes as the base keeps v below 4 for any chunk size
  if constexpr (M::kLanes) M::template st_lanes<4>(w + 12 * (gi >> 2), (uint32_t)(gi & 3), q);
  else st_wire<QB>(w + gi * QB, q);
  if ((gi & 7) == 0) w[kern::mx_scale_off(F, cb, gi >> 3)] = (char)sc.byte;
}

}  // namespace dev
}  // namespace pdcc
