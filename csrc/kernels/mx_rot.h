// Random Hadamard rotation for the block-scaled wire formats (docs/collectives.md "Hadamard rotation").
// Host and device, no HIP runtime call: the kernels (mx_wire.hip) and tests/native/mx_rot_check.cpp read
// the one definition.
//
// A 32-element block x is rotated to R x = H diag(s) x before it is quantized and back with
// R^-1 d = diag(s) (2^-5 H d) after it is dequantized: H[i][j] = (-1)^popcount(i & j) is the unnormalized
// Sylvester-Hadamard matrix (H H = 32 I), s_j = -1 where bit j of the call's sign word is set. The
// butterfly below is the definition of the product with H: its order fixes the f32 roundings.
#pragma once
#include <stdint.h>
#include <string.h>

#include "mx_sr.h"

namespace pdcc {
namespace kern {

constexpr uint32_t kMxRotStream = 0x52484431u;  // "RHD1": the stream of the sign word, no rank's stream

// the sign word of a call: bit j belongs to position j of every block
PDCC_SR_HD uint32_t mx_rot_signs(uint64_t seed) { return mx_sr_word(mx_sr_key(seed, kMxRotStream), 0); }

// ---- the plain host form of both transforms on one block of 32 floats (the kernels spread the same
// operations over the lanes of a block)
inline uint32_t mx_rot_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
inline float mx_rot_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline void mx_rot_flip(float* y, uint32_t signs) {
  for (int j = 0; j < 32; ++j) y[j] = mx_rot_float(mx_rot_bits(y[j]) ^ (((signs >> j) & 1u) << 31));
}
inline void mx_rot_butterfly(float* y) {
  for (int h = 1; h < 32; h <<= 1)
    for (int j = 0; j < 32; ++j)
      if ((j & h) == 0) {
        const volatile float a = y[j], b = y[j + h];  // (volatile: one f32 operation each, nothing fused)
        y[j] = a + b;
        y[j + h] = a - b;
      }
}
inline void mx_rot_forward(float* y, uint32_t signs) {
  mx_rot_flip(y, signs);
  mx_rot_butterfly(y);
}
inline void mx_rot_inverse(float* y, uint32_t signs) {
  mx_rot_butterfly(y);
  for (int j = 0; j < 32; ++j) y[j] = y[j] * 0.03125f;
  mx_rot_flip(y, signs);
}

}  // namespace kern
}  // namespace pdcc
