// Stochastic rounding for the block-scaled wire formats (docs/collectives.md "Stochastic rounding").
// Host and device, no HIP runtime call: the kernels (mx_wire.hip) and tests/native/mx_sr_check.cpp read
// the one definition.
//
// Two things live here, both plain integer arithmetic:
//   * the counter-based random words: mx_sr_mix, the key of a call, the word of an element index;
//   * the rounding of one scaled value s = x 2^-e (an f32, given as its bits) with one 32-bit word u
//     to an e4m3 byte, an e2m1 code or an e2m3 code: with lo <= |s| < hi the neighbouring magnitudes of the format's
//     grid, t = (|s| - lo) / (hi - lo) and T = floor(t 2^32), the magnitude is hi iff u < T.
//
// The grids are ordered like their codes (sign bit aside), so hi is code(lo) + 1, and each is a
// floating-point grid with MB mantissa bits whose smallest normal magnitude has the f32 exponent field
// FMIN: e4m3 has MB = 3 and FMIN = 121 (2^-6), e2m1 has MB = 1 and FMIN = 127 (1), e2m3 has MB = 3 and
// FMIN = 127. With M the 24-bit
// significand of |s| and d = max(0, FMIN - field), the grid step at |s| is 2^sh units of M's last
// place, sh = 23 - MB + d: lo's code is ((field - FMIN) << MB for a normal, 0 below) + (M >> sh), and
// t is the sh bits under it. In the normal binades sh = 20 (e4m3, e2m3) or 22 (e2m1), so T = frac << (32 - sh)
// holds t exactly; further down T is the floor of a longer fraction and 0 from 2^-33 of a step on.
// An f32 subnormal lands there whatever its significand is taken to be.
//
// |s| must not exceed the format's largest magnitude (448, 6, 7.5): the block scale sees to that, and the
// largest magnitude itself is on the grid, so nothing ever rounds past it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDCC_SR_HD __host__ __device__ inline
#else
#define PDCC_SR_HD inline
#endif

namespace pdcc {
namespace kern {

PDCC_SR_HD uint32_t mx_sr_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// key of a call from its 64-bit seed and its 32-bit stream
PDCC_SR_HD uint32_t mx_sr_key(uint64_t seed, uint32_t stream) {
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  return mx_sr_mix(mx_sr_mix(mx_sr_mix(lo ^ 0x9E3779B9u) + hi) + stream);
}

// key of the 2^32 indices that share the high word h
PDCC_SR_HD uint32_t mx_sr_key_h(uint32_t k, uint32_t h) { return h == 0 ? k : mx_sr_mix(k + h); }

// word of the low half of an index under its high word's key
PDCC_SR_HD uint32_t mx_sr_word_lo(uint32_t kh, uint32_t i_lo) { return mx_sr_mix(i_lo ^ kh); }

PDCC_SR_HD uint32_t mx_sr_word(uint32_t k, uint64_t i) {
  return mx_sr_word_lo(mx_sr_key_h(k, (uint32_t)(i >> 32)), (uint32_t)i);
}

// code of the magnitude lo and T = floor(t 2^32) for the f32 bits `a` of |s|
template <int MB, int FMIN>
PDCC_SR_HD void mx_sr_split(uint32_t a, uint32_t& lo, uint32_t& T) {
  const uint32_t field = a >> 23;
  const uint32_t M = (a & 0x7fffffu) | 0x800000u;
  const bool normal = field >= (uint32_t)FMIN;
  uint32_t d = normal ? 0u : (uint32_t)FMIN - field;
  if (d > 40u) d = 40u;  // (T and lo are 0 from d = 33 + MB on: M < 2^24)
  const uint32_t sh = 23u - MB + d;  // 20 .. 63
  const uint32_t base = normal ? (field - (uint32_t)FMIN) << MB : 0u;
  lo = base + (sh < 32u ? M >> sh : 0u);
  const uint32_t frac = sh < 32u ? M & ((1u << sh) - 1u) : M;
  T = sh <= 32u ? frac << (32u - sh) : frac >> (sh - 32u);
}

// s (f32 bits, |s| <= 448) and a word -> float8_e4m3fn byte
PDCC_SR_HD uint32_t mx_sr_e4m3(uint32_t s_bits, uint32_t u) {
  uint32_t lo, T;
  mx_sr_split<3, 121>(s_bits & 0x7fffffffu, lo, T);
  return (((s_bits >> 31) << 7) | (lo + (u < T ? 1u : 0u))) & 0xffu;
}

// s (f32 bits, |s| <= 6) and a word -> e2m1 code, the sign in bit 3
PDCC_SR_HD uint32_t mx_sr_e2m1(uint32_t s_bits, uint32_t u) {
  uint32_t lo, T;
  mx_sr_split<1, 127>(s_bits & 0x7fffffffu, lo, T);
  return (((s_bits >> 31) << 3) | (lo + (u < T ? 1u : 0u))) & 0xfu;
}

// s (f32 bits, |s| <= 7.5) and a word -> e2m3 code, the sign in bit 5
PDCC_SR_HD uint32_t mx_sr_e2m3(uint32_t s_bits, uint32_t u) {
  uint32_t lo, T;
  mx_sr_split<3, 127>(s_bits & 0x7fffffffu, lo, T);
  return (((s_bits >> 31) << 5) | (lo + (u < T ? 1u : 0u))) & 0x3fu;
}

}  // namespace kern
}  // namespace pdcc
