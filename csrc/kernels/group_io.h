// Groups of elements for the streaming f32 / bf16 / f16 kernels (grad_clip.hip, adamw.hip): one 8- or 16-byte
// vector access per group, widened to f32 on the way in and rounded once on the way out, the element path for
// misaligned bases and for the group that straddles the end, and the clip coefficient both kernels read.
#pragma once
#include "dev_common.h"

namespace pdcc {
namespace dev {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

template <DType DT>
__device__ __forceinline__ float widen_bits(uint32_t b) {
  if constexpr (DT == DType::BF16) return bf16_to_f32((uint16_t)b);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}
template <DType DT>
__device__ __forceinline__ uint32_t narrow_bits(float f) {
  if constexpr (DT == DType::BF16) return f32_to_bf16(f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}

// f rounded once to DT and widened again: the value a store of DT leaves behind
template <DType DT>
__device__ __forceinline__ float round_as(float f) {
  if constexpr (DT == DType::F32) return f;
  else return widen_bits<DT>(narrow_bits<DT>(f));
}

// N elements of DT from N * sizeof(element) bytes (8 or 16, so aligned); NT: non-temporal (read once)
template <DType DT, int N, bool NT = true>
__device__ __forceinline__ void load_group(const char* p, float* f) {
  constexpr int kBytes = N * (int)sizeof(typename Tr<DT>::S);
  static_assert(kBytes == 8 || kBytes == 16, "a group is one 8- or 16-byte access");
  uint32_t w[kBytes / 4];
  if constexpr (kBytes == 16) {
    const v4u x = NT ? __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p)) : *reinterpret_cast<const v4u*>(p);
    w[0] = x[0], w[1] = x[1], w[2] = x[2], w[3] = x[3];
  } else {
    const v2u x = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p)) : *reinterpret_cast<const v2u*>(p);
    w[0] = x[0], w[1] = x[1];
  }
#pragma unroll
  for (int i = 0; i < kBytes / 4; ++i) {
    if constexpr (DT == DType::F32) f[i] = __uint_as_float(w[i]);
    else f[2 * i] = widen_bits<DT>(w[i] & 0xffffu), f[2 * i + 1] = widen_bits<DT>(w[i] >> 16);
  }
}

// the output side of a group: 16 bytes, or 8 (four 16-bit elements next to a 16-byte f32 side); NT: non-temporal
template <DType DT, int N, bool NT = false>
__device__ __forceinline__ void store_group(char* p, const float* f) {
  constexpr int kBytes = N * (int)sizeof(typename Tr<DT>::S);
  static_assert(kBytes == 8 || kBytes == 16, "the output side of a group is 8 or 16 bytes");
  uint32_t w[kBytes / 4];
#pragma unroll
  for (int i = 0; i < kBytes / 4; ++i) {
    if constexpr (DT == DType::F32) w[i] = __float_as_uint(f[i]);
    else w[i] = narrow_bits<DT>(f[2 * i]) | (narrow_bits<DT>(f[2 * i + 1]) << 16);
  }
  if constexpr (kBytes == 16) {
    const v4u x = {w[0], w[1], w[2], w[3]};
    if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<v4u*>(p));
    else *reinterpret_cast<v4u*>(p) = x;
  } else {
    const v2u x = {w[0], w[1]};
    if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<v2u*>(p));
    else *reinterpret_cast<v2u*>(p) = x;
  }
}

// elements [i, i + N) of the tensor, those at or past `numel` as +0 and never read
template <DType DT, int N>
__device__ __forceinline__ void load_elems(const char* base, size_t i, size_t numel, float* f) {
  using S = typename Tr<DT>::S;
#pragma unroll
  for (int j = 0; j < N; ++j) f[j] = i + j < numel ? Tr<DT>::in(reinterpret_cast<const S*>(base)[i + j]) : 0.0f;
}
template <DType DT, int N>
__device__ __forceinline__ void store_elems(char* base, size_t i, size_t numel, const float* f) {
  using S = typename Tr<DT>::S;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (i + j < numel) reinterpret_cast<S*>(base)[i + j] = Tr<DT>::out(f[j]);
}

// torch.nn.utils.clip_grad_norm_'s coefficient, in f32 from the f64 total; a NaN stays a NaN
__device__ __forceinline__ float clip_coef(const double* total, float max_norm) {
#pragma clang fp contract(off)
  const float norm = (float)sqrt(*total);
  const float c = max_norm / (norm + 1e-6f);
  return (c < 1.0f || c != c) ? c : 1.0f;
}

}  // namespace dev
}  // namespace pdcc
