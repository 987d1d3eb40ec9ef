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
//   mx_quantize_list / mx_dequantize_list: the dealt wire of a list of tensors read and written where they
//                  are, every tensor starting a fresh block (docs/collectives.md "Tensor-list layout"); the
//                  one pair of kernels that uses LDS, for the table of the tensors' descriptors
//
// The options of a call (MxOpts, kernel_api.h) pick the instantiation:
//   residual       the EF instantiations of the quantizers (quantize, its shard and list forms, reduce), which
//                  add an f32 residual before they quantize and leave what the quantizer dropped in it
//                  (docs/collectives.md "Error feedback"); per f32 element quantize then reads 8 and
//                  writes 4 + 33/32 bytes instead of reading 4
//   sr             the SR instantiations of the quantizers, which round the payload stochastically
//                  (docs/collectives.md "Stochastic rounding", mx_sr.h); they move the bytes of the plain kernels
//   rot_signs      the ROT instantiations of everything that touches the tensor (all but reduce), which
//                  rotate every block (docs/collectives.md "Hadamard rotation", mx_rot.h)
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
// Every kernel is a template over the format (MxFmt, mx_fmt.h): the formats share the lane layout on the
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
// |s| <= 7.5 and the code is its low five bits and its sign (MxFmt<FP6_E2M3>). e is clamped to
// [-123, 126].
#include <algorithm>
#include <type_traits>

#include "dev_common.h"
#include "mx_block.h"
#include "mx_fmt.h"
#include "mx_layout.h"
#include "mx_rot.h"
#include "mx_sr.h"

namespace pdcc {
namespace dev {

namespace {

using kern::MxFormat;
constexpr int kMxUnroll = 4;  // independent 16-B loads in flight per lane (quantize / dequantize)

// (the block amax, the scale rule and the packed FP8 converts with the scale applied: mx_block.h)

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

// (MxFmt<F> -- the scale rule, pack / unpack and the payload accesses of a format -- and ld_wire / st_wire: mx_fmt.h)

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

// ---------------------------------------------------------------------------- tensor lists
// Quantize and dequantize in the tensor-list layout (mx_layout.h): the dealt wire of a virtual tensor whose
// blocks belong to up to kMaxMxListDescs tensors of this launch, read and written where they lie. The wire
// side is that of the dealt kernels. The tensor side goes through a descriptor table: the kernarg copy is
// spread to LDS once per workgroup, a span (kMxUnroll * 256 vectors of one chunk) finds the tensor of its
// first block by binary search, and every lane then walks its own cursor forward -- a span lies inside one
// tensor almost always, and then that walk is one LDS read per vector that fails its test.
//
// A launch owns the blocks [g0, g1) of the virtual tensor (the host splits long lists at tensor boundaries,
// which are block boundaries): [g0, end) belong to its tensors, [end, g1) are padding blocks of the wire
// (quantize only). Spans are cut per chunk, span s is the vectors from (s % spc) * kMxUnroll * 256 on of
// chunk s / spc, so a span at an edge of the range is shared with the neighbouring launch and each masks
// the other's blocks. Whole blocks are live or not, so the lanes that share a DPP exchange run together.
struct MxListDesc {
  const char* base;
  uint64_t numel;
  uint32_t first;  // B_i
};
struct MxListArgs {
  MxListDesc d[kern::kMaxMxListDescs];
  uint32_t n, g0, g1, end;
};
struct MxListTable {
  uint32_t first[kern::kMaxMxListDescs + 1];  // first[n] = end
  const char* base[kern::kMaxMxListDescs];
  uint64_t numel[kern::kMaxMxListDescs];
};
__device__ __forceinline__ void list_table_load(const MxListArgs& a, MxListTable& t) {
  if (threadIdx.x < a.n) {
    t.first[threadIdx.x] = a.d[threadIdx.x].first;
    t.base[threadIdx.x] = a.d[threadIdx.x].base;
    t.numel[threadIdx.x] = a.d[threadIdx.x].numel;
  }
  if (threadIdx.x == 0) t.first[a.n] = a.end;
  __syncthreads();
}
// the last descriptor that starts at or before block g (g >= first[0]); 0 for an empty table
__device__ __forceinline__ uint32_t list_find(const MxListTable& t, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (t.first[mid] <= g) lo = mid + 1;
    else hi = mid;
  }
  return lo ? lo - 1 : 0;
}
// A lane's place in the list: the tensor of block g (a block below `end`; g never decreases between calls),
// and how many of the EPL elements from the lane's `place` on the tensor has (0 .. EPL).
struct MxListCursor {
  uint32_t idx;
  template <int EPL>
  __device__ __forceinline__ uint32_t seek(const MxListTable& t, uint32_t n, uint32_t g, uint32_t place, uint64_t* el) {
    while (idx + 1 < n && g >= t.first[idx + 1]) ++idx;
    *el = (uint64_t)(g - t.first[idx]) * kern::kMxBlock + place * EPL;  // first element, in the tensor
    const uint64_t numel = t.numel[idx];
    return *el >= numel ? 0u : (numel - *el >= (uint64_t)EPL ? (uint32_t)EPL : (uint32_t)(numel - *el));
  }
};

// EF: `res` holds one float per virtual position, 32 per block, so a lane's EPL floats are always aligned
// vectors; the positions of a last block past its tensor's end are read like the others and written as
// +0. Padding blocks have no residual. SR: the word index is `sr_base` plus the virtual position.
template <MxFormat F, DType DT, bool EF, bool SR, bool ROT>
__global__ __launch_bounds__(256) void k_mx_quantize_list(const MxListArgs a, char* __restrict__ wire, uint32_t cb,
                                                          uint32_t spc, uint32_t s0, uint32_t s1,
                                                          float* __restrict__ res, uint32_t sr_key, uint64_t sr_base,
                                                          uint32_t rot_signs) {
  static_assert(!(EF && SR), "error feedback and stochastic rounding are alternatives");
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  using M = MxFmt<F>;
  constexpr int QB = EPL * M::kPayload / kern::kMxBlock, QW = M::template kWords<EPL>;
  __shared__ MxListTable t;
  list_table_load(a, t);
  const uint32_t nvec = cb * LPB;
  for (uint32_t s = s0 + blockIdx.x; s < s1; s += gridDim.x) {
    const uint32_t chunk = s / spc, vs = (s - chunk * spc) * (256u * kMxUnroll);
    char* __restrict__ w = wire + (size_t)chunk * kern::mx_chunk_bytes(F, cb);
    const uint32_t gb = chunk * cb;  // the chunk's first block
    const uint32_t gs = gb + vs / LPB;
    MxListCursor cur{list_find(t, a.n, gs > a.g0 ? gs : a.g0)};
    S sv[kMxUnroll][EPL];
    float r[EF ? kMxUnroll : 1][EPL];
    uint32_t have[EF ? kMxUnroll : 1];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = vs + threadIdx.x + u * 256u, g = gb + v / LPB;
      __builtin_memset(sv[u], 0, sizeof(sv[u]));
      if constexpr (EF) {
        __builtin_memset(r[u], 0, sizeof(r[u]));
        have[u] = 0u;
      }
      if (v < nvec && g >= a.g0 && g < a.end) {
        uint64_t el;
        const uint32_t nv = cur.template seek<EPL>(t, a.n, g, v % LPB, &el);
        const char* p = t.base[cur.idx] + el * sizeof(S);
        if (nv == (uint32_t)EPL && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
          const uint4 x = *reinterpret_cast<const uint4*>(p);
          __builtin_memcpy(sv[u], &x, 16);
        } else {
          // a misaligned tensor, or its last vector: elements past the end count as +0 and are never read
#pragma unroll
          for (int i = 0; i < EPL; ++i)
            if ((uint32_t)i < nv) sv[u][i] = reinterpret_cast<const S*>(p)[i];
        }
        if constexpr (EF) {
          have[u] = nv;
          const float* rp = res + (size_t)g * kern::kMxBlock + (v % LPB) * EPL;
#pragma unroll
          for (int j = 0; j < EPL / 4; ++j) {
            const uint4 y = *reinterpret_cast<const uint4*>(rp + 4 * j);
            __builtin_memcpy(&r[u][4 * j], &y, 16);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = vs + threadIdx.x + u * 256u, g = gb + v / LPB;
      if (v >= nvec) break;  // (whole waves leave together: nvec and every span start are multiples of 64)
      if (g < a.g0 || g >= a.g1) continue;  // (a neighbouring launch's blocks)
      float f[EPL];
      uint32_t am = 0;
      if constexpr (ROT) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) f[i] = T::in(sv[u][i]);
        rot_forward<EPL>(f, rot_signs, v % LPB);
      }
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        if constexpr (!ROT) f[i] = T::in(sv[u][i]);
        if constexpr (EF) f[i] += r[u][i];
        const uint32_t ab = abs_bits(f[i]);
        am = ab > am ? ab : am;
      }
      const MxScale sc = M::scale(group_max<LPB>(am));
      uint32_t q[QW];
      const uint64_t pos = (uint64_t)g * kern::kMxBlock + (v % LPB) * EPL;  // the lane's virtual position
      if constexpr (SR) M::template pack_sr<EPL>(f, sc, q, SrWords(sr_key, sr_base + pos, EPL));
      else M::template pack<EPL>(f, sc, q);
      if constexpr (M::kLanes) M::template st_lanes<EPL>(w, v, q);
      else st_wire<QB>(w + (size_t)v * QB, q);
      if (v % LPB == 0) w[kern::mx_scale_off(F, cb, v / LPB)] = (char)sc.byte;
      if constexpr (EF) {
        if (g < a.end) {
          float d[EPL];
          M::template unpack<EPL>(q, mx_scale_value(sc.byte), d);
#pragma unroll
          for (int i = 0; i < EPL; ++i) d[i] = (uint32_t)i < have[u] ? ef_residual(f[i], d[i]) : 0.0f;
#pragma unroll
          for (int j = 0; j < EPL / 4; ++j) {
            uint4 y;
            __builtin_memcpy(&y, &d[4 * j], 16);
            *reinterpret_cast<uint4*>(res + pos + 4 * j) = y;
          }
        }
      }
    }
  }
}

// Every lane of a tensor's blocks loads, converts and (ROT) takes part in the rotation; only the stores are
// masked, by the tensor's end, and go out as one vector where the tensor is 16-byte aligned.
template <MxFormat F, DType DT, bool ROT>
__global__ __launch_bounds__(256) void k_mx_dequantize_list(const MxListArgs a, const char* __restrict__ wire,
                                                            uint32_t cb, uint32_t spc, uint32_t s0, uint32_t s1,
                                                            uint32_t rot_signs) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  using M = MxFmt<F>;
  constexpr int QB = EPL * M::kPayload / kern::kMxBlock, QW = M::template kWords<EPL>;
  __shared__ MxListTable t;
  list_table_load(a, t);
  const uint32_t nvec = cb * LPB;
  for (uint32_t s = s0 + blockIdx.x; s < s1; s += gridDim.x) {
    const uint32_t chunk = s / spc, vs = (s - chunk * spc) * (256u * kMxUnroll);
    const char* __restrict__ w = wire + (size_t)chunk * kern::mx_chunk_bytes(F, cb);
    const uint32_t gb = chunk * cb;
    const uint32_t gs = gb + vs / LPB;
    MxListCursor cur{list_find(t, a.n, gs > a.g0 ? gs : a.g0)};
    uint32_t q[kMxUnroll][QW];
    uint32_t sb[kMxUnroll];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = vs + threadIdx.x + u * 256u, g = gb + v / LPB;
      sb[u] = 127u;
#pragma unroll
      for (int d = 0; d < QW; ++d) q[u][d] = 0u;
      if (v < nvec && g >= a.g0 && g < a.end) {
        if constexpr (M::kLanes) M::template ld_lanes<EPL>(w, v, q[u]);
        else ld_wire<QB>(w + (size_t)v * QB, q[u]);
        sb[u] = (uint8_t)w[kern::mx_scale_off(F, cb, v / LPB)];
      }
    }
    if constexpr (M::kLanes) {  // (v % 4 is the lane's place in its hardware quad: vs is a multiple of 64)
#pragma unroll
      for (int u = 0; u < kMxUnroll; ++u) M::template gather<EPL>(vs + threadIdx.x + u * 256u, q[u]);
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = vs + threadIdx.x + u * 256u, g = gb + v / LPB;
      if (v >= nvec) break;
      if (g < a.g0 || g >= a.end) continue;
      float f[EPL];
      M::template unpack<EPL>(q[u], mx_scale_value(sb[u]), f);
      if constexpr (ROT) rot_inverse<EPL>(f, rot_signs, v % LPB);
      S o[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i) o[i] = T::out(f[i]);
      uint64_t el;
      const uint32_t nv = cur.template seek<EPL>(t, a.n, g, v % LPB, &el);
      char* p = const_cast<char*>(t.base[cur.idx]) + el * sizeof(S);
      if (nv == (uint32_t)EPL && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        uint4 x;
        __builtin_memcpy(&x, o, 16);
        *reinterpret_cast<uint4*>(p) = x;
      } else {
#pragma unroll
        for (int i = 0; i < EPL; ++i)
          if ((uint32_t)i < nv) reinterpret_cast<S*>(p)[i] = o[i];
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
bool mx_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }  // (null counts as aligned)
// What every launch checks: the format is one of the three; cb is a multiple of 16, and a chunk's lanes are
// counted in 32 bits; a quantizer takes a residual or stochastic rounding, not both, and the other kernels
// neither; the residual and the buffers `a` and `b` are 16-byte aligned.
bool mx_args_ok(const MxOpts& o, bool quantizer, size_t cb, const void* a, const void* b) {
  const bool fmt = o.fmt == MxFormat::FP8_E4M3 || o.fmt == MxFormat::FP4_E2M1 || o.fmt == MxFormat::FP6_E2M3;
  const bool opts = quantizer ? !(o.residual && o.sr) : !o.residual && !o.sr;
  return fmt && opts && cb > 0 && cb % kMxScaleAlign == 0 && cb <= (size_t(1) << 27) && mx_al16(o.residual) &&
         mx_al16(a) && mx_al16(b);
}
size_t mx_esize(DType t) { return t == DType::F32 ? 4 : 2; }
bool mx_dtype_ok(DType t) { return t == DType::F32 || t == DType::BF16 || t == DType::F16; }
bool mx_chunks_ok(size_t nchunks) { return nchunks > 0 && nchunks <= 65535; }  // (a chunk is a grid row)
// the shard arguments (after mx_args_ok): m elements per shard fit the chunk, and the whole tensor's size is a size_t
bool mx_shards_ok(size_t m, size_t cb, size_t nchunks) { return m > 0 && m <= cb * kMxBlock && mx_chunks_ok(nchunks); }
// the sources and the op of reduce and fold
bool mx_fold_ok(int nsrc, RedOp op, int avg_div) {
  return nsrc >= 1 && nsrc <= kMaxRanks && (op == RedOp::SUM || (op == RedOp::AVG && avg_div >= 1));
}
// the word indices index_offset .. index_offset + numel of a stochastic call fit 64 bits
bool mx_sr_fits(const MxOpts& o, size_t numel) { return !o.sr || o.sr->index_offset + numel >= o.sr->index_offset; }
dim3 mx_stream_grid(size_t cb, DType t, size_t nchunks) {
  const int lpb = t == DType::F32 ? 8 : 4;
  return dim3(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
}
// key and index base of a stochastic call (mx_sr.h); zeros without one
struct MxSrKey {
  uint32_t key;
  uint64_t base;
};
MxSrKey mx_sr_key_of(const MxOpts& o) {
  return o.sr ? MxSrKey{mx_sr_key(o.sr->seed, o.sr->stream), o.sr->index_offset} : MxSrKey{0u, 0u};
}

// ---- from a runtime value to a template argument: each helper calls the generic `fn` with the value as a tag (an
// integral_constant; PDCC_V reads it back), so a launch function below is nested lifts around one launch.
// The callers have checked the values: what is not listed cannot arrive.
template <auto V>
using MxTag = std::integral_constant<decltype(V), V>;
#define PDCC_V(tag) decltype(tag)::value
template <class Fn>
void mx_lift_fmt(MxFormat f, Fn&& fn) {
  switch (f) {
    case MxFormat::FP4_E2M1: return fn(MxTag<MxFormat::FP4_E2M1>{});
    case MxFormat::FP6_E2M3: return fn(MxTag<MxFormat::FP6_E2M3>{});
    default: return fn(MxTag<MxFormat::FP8_E4M3>{});
  }
}
template <class Fn>
void mx_lift_dtype(DType t, Fn&& fn) {
  switch (t) {
    case DType::F32: return fn(MxTag<DType::F32>{});
    case DType::BF16: return fn(MxTag<DType::BF16>{});
    default: return fn(MxTag<DType::F16>{});
  }
}
template <class Fn>
void mx_lift_bool(bool b, Fn&& fn) {
  if (b) fn(MxTag<true>{});
  else fn(MxTag<false>{});
}
template <class Fn>
void mx_lift_nsrc(int nsrc, Fn&& fn) {
  switch (nsrc) {
    case 1: return fn(MxTag<1>{});
    case 2: return fn(MxTag<2>{});
    case 3: return fn(MxTag<3>{});
    case 4: return fn(MxTag<4>{});
    case 5: return fn(MxTag<5>{});
    case 6: return fn(MxTag<6>{});
    case 7: return fn(MxTag<7>{});
    default: return fn(MxTag<8>{});
  }
}
// what a quantizer does besides rounding to nearest: nothing, error feedback (a residual) or stochastic
// rounding -- one tag of three values, because the kernels have no instantiation with both
enum class MxMode { PLAIN, EF, SR };
template <class Fn>
void mx_lift_mode(const MxOpts& o, Fn&& fn) {
  if (o.sr) fn(MxTag<MxMode::SR>{});
  else if (o.residual) fn(MxTag<MxMode::EF>{});
  else fn(MxTag<MxMode::PLAIN>{});
}
// the dealt kernel, or the shard one with or without vectors (there is no dealt kernel without them): 16-byte
// vectors when every shard, and its slice of a residual, starts 16-byte aligned
enum class MxLayout { DEALT, SHARD_VEC, SHARD_SCALAR };
MxLayout mx_shard_layout(size_t m, DType t) {
  return m * mx_esize(t) % 16 == 0 ? MxLayout::SHARD_VEC : MxLayout::SHARD_SCALAR;
}
template <class Fn>
void mx_lift_layout(MxLayout l, Fn&& fn) {
  switch (l) {
    case MxLayout::DEALT: return fn(MxTag<MxLayout::DEALT>{});
    case MxLayout::SHARD_VEC: return fn(MxTag<MxLayout::SHARD_VEC>{});
    default: return fn(MxTag<MxLayout::SHARD_SCALAR>{});
  }
}

// ---- one launch function per kernel family
// quantize / dequantize of `numel` elements in all: dealt, or shards of `m` elements (the dealt kernels ignore m)
hipError_t mx_quantize_launch(MxLayout layout, const void* src, size_t numel, size_t m, DType t, void* wire, size_t cb,
                              size_t nchunks, hipStream_t stream, const MxOpts& o) {
  const dim3 grid = mx_stream_grid(cb, t, nchunks);
  const char* s = static_cast<const char*>(src);
  char* w = static_cast<char*>(wire);
  const MxSrKey sr = mx_sr_key_of(o);
  const uint32_t c = (uint32_t)cb, signs = o.rot_signs ? *o.rot_signs : 0u;
  mx_lift_fmt(o.fmt, [&](auto f) {
    mx_lift_dtype(t, [&](auto dt) {
      mx_lift_layout(layout, [&](auto l) {
        mx_lift_mode(o, [&](auto mode) {
          mx_lift_bool(o.rot_signs != nullptr, [&](auto rot) {
            constexpr bool shard = PDCC_V(l) != MxLayout::DEALT, vec = PDCC_V(l) != MxLayout::SHARD_SCALAR;
            constexpr bool ef = PDCC_V(mode) == MxMode::EF, st = PDCC_V(mode) == MxMode::SR;
            hipLaunchKernelGGL((dev::k_mx_quantize<PDCC_V(f), PDCC_V(dt), shard, vec, ef, st, PDCC_V(rot)>), grid, dim3(256),
                               0, stream, s, numel, w, c, m, o.residual, sr.key, sr.base, signs);
          });
        });
      });
    });
  });
  return hipGetLastError();
}
hipError_t mx_dequantize_launch(MxLayout layout, const void* wire, size_t cb, size_t nchunks, void* dst, size_t numel,
                                size_t m, DType t, hipStream_t stream, const MxOpts& o) {
  const dim3 grid = mx_stream_grid(cb, t, nchunks);
  const char* w = static_cast<const char*>(wire);
  char* d = static_cast<char*>(dst);
  const uint32_t c = (uint32_t)cb, signs = o.rot_signs ? *o.rot_signs : 0u;
  mx_lift_fmt(o.fmt, [&](auto f) {
    mx_lift_dtype(t, [&](auto dt) {
      mx_lift_layout(layout, [&](auto l) {
        mx_lift_bool(o.rot_signs != nullptr, [&](auto rot) {
          constexpr bool shard = PDCC_V(l) != MxLayout::DEALT, vec = PDCC_V(l) != MxLayout::SHARD_SCALAR;
          hipLaunchKernelGGL((dev::k_mx_dequantize<PDCC_V(f), PDCC_V(dt), shard, vec, PDCC_V(rot)>), grid, dim3(256), 0,
                             stream, w, c, d, numel, m, signs);
        });
      });
    });
  });
  return hipGetLastError();
}

// ---- tensor lists: one launch per kMaxMxListDescs tensors that own a block
// Quantize (QUANT) or dequantize the list in launches of up to kMaxMxListDescs tensors. A launch owns the
// blocks from its first tensor's to the next launch's; the last one of a quantize also owns the padding
// blocks up to cb * nchunks, and a list without a block is one launch of padding alone.
template <bool QUANT>
hipError_t mx_list_run(const MxListTensor* ts, size_t k, DType t, char* wire, size_t cb, size_t nchunks,
                       hipStream_t stream, const MxOpts& opts) {
  if (!mx_args_ok(opts, QUANT, cb, wire, nullptr) || !mx_dtype_ok(t) || !mx_chunks_ok(nchunks)) return hipErrorInvalidValue;
  if (k > 65535 || (k && !ts) || !mx_sr_fits(opts, mx_list_numel(ts, k))) return hipErrorInvalidValue;
  MxOpts o = opts;
  if (mx_list_blocks(ts, k) == 0 && !o.sr) o.residual = nullptr;  // (no block: no residual to update, the wire is all padding blocks)
  const MxSrKey sr = mx_sr_key_of(o);
  const uint32_t signs = o.rot_signs ? *o.rot_signs : 0u;
  const uint64_t total = (uint64_t)cb * nchunks;  // blocks on the wire; the kernels count them in 32 bits
  if (total >= (uint64_t(1) << 32) || mx_list_blocks(ts, k) > total) return hipErrorInvalidValue;
  for (size_t i = 0; i < k; ++i)
    if (ts[i].numel && (!ts[i].base || reinterpret_cast<uintptr_t>(ts[i].base) % mx_esize(t))) return hipErrorInvalidValue;
  const uint32_t lpb = t == DType::F32 ? 8 : 4, span = 256u * dev::kMxUnroll;
  const uint32_t spc = (uint32_t)(((uint64_t)cb * lpb + span - 1) / span);  // spans per chunk
  const auto span_of = [&](uint64_t g) { return (uint32_t)(g / cb * spc + g % cb * lpb / span); };
  size_t i = 0;
  uint64_t first = 0;  // B_i
  bool more = true;
  while (more) {
    dev::MxListArgs a{};
    a.g0 = (uint32_t)first;
    for (; i < k && a.n < (uint32_t)kMaxMxListDescs; ++i) {
      if (ts[i].numel == 0) continue;  // (owns no block)
      a.d[a.n++] = dev::MxListDesc{static_cast<const char*>(ts[i].base), (uint64_t)ts[i].numel, (uint32_t)first};
      first += mx_blocks(ts[i].numel);
    }
    while (i < k && ts[i].numel == 0) ++i;
    more = i < k;
    a.end = (uint32_t)first;
    a.g1 = QUANT && !more ? (uint32_t)total : a.end;
    if (a.g1 == a.g0) break;  // (a dequantize without a block)
    const uint32_t s0 = span_of(a.g0), s1 = span_of(a.g1 - 1) + 1;
    const dim3 grid((uint32_t)std::min<uint64_t>(s1 - s0, dev::kMxGridStream));
    const uint32_t c = (uint32_t)cb;
    mx_lift_fmt(o.fmt, [&](auto f) {
      mx_lift_dtype(t, [&](auto dt) {
        mx_lift_bool(o.rot_signs != nullptr, [&](auto rot) {
          if constexpr (QUANT) {
            mx_lift_mode(o, [&](auto mode) {
              constexpr bool ef = PDCC_V(mode) == MxMode::EF, st = PDCC_V(mode) == MxMode::SR;
              hipLaunchKernelGGL((dev::k_mx_quantize_list<PDCC_V(f), PDCC_V(dt), ef, st, PDCC_V(rot)>), grid, dim3(256), 0,
                                 stream, a, wire, c, spc, s0, s1, o.residual, sr.key, sr.base, signs);
            });
          } else {
            hipLaunchKernelGGL((dev::k_mx_dequantize_list<PDCC_V(f), PDCC_V(dt), PDCC_V(rot)>), grid, dim3(256), 0, stream, a,
                               wire, c, spc, s0, s1, signs);
          }
        });
      });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// reduce: lanes per block from the payload bytes of a lane, 16 (FP6: 24)
hipError_t mx_reduce_launch(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out,
                            hipStream_t stream, const MxOpts& o) {
  const char* in = static_cast<const char*>(wire_in);
  char* out = static_cast<char*>(wire_out);
  const uint32_t c = (uint32_t)cb, key = mx_sr_key_of(o).key;
  const int lpb = o.fmt == MxFormat::FP8_E4M3 ? 2 : 1;
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, 1, 1, dev::kMxGridReduce));
  mx_lift_fmt(o.fmt, [&](auto f) {
    mx_lift_bool(op == RedOp::AVG, [&](auto avg) {
      mx_lift_mode(o, [&](auto mode) {
        mx_lift_nsrc(nsrc, [&](auto n) {
          constexpr bool ef = PDCC_V(mode) == MxMode::EF, st = PDCC_V(mode) == MxMode::SR;
          hipLaunchKernelGGL((dev::k_mx_reduce<PDCC_V(f), PDCC_V(n), PDCC_V(avg), ef, st>), grid, dim3(256), 0, stream, in, c,
                             avg_div, out, o.residual, key);
        });
      });
    });
  });
  return hipGetLastError();
}
hipError_t mx_fold_launch(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* dst, size_t numel, DType t,
                          hipStream_t stream, const MxOpts& o) {
  const char* in = static_cast<const char*>(wire_in);
  char* d = static_cast<char*>(dst);
  const uint32_t c = (uint32_t)cb, signs = o.rot_signs ? *o.rot_signs : 0u;
  const uint64_t epl = 16 / mx_esize(t), nvec = (numel + epl - 1) / epl;
  mx_lift_fmt(o.fmt, [&](auto f) {
    mx_lift_dtype(t, [&](auto dt) {
      mx_lift_nsrc(nsrc, [&](auto n) {
        mx_lift_bool(op == RedOp::AVG, [&](auto avg) {
          mx_lift_bool(o.rot_signs != nullptr, [&](auto rot) {
            const dim3 grid(dev::mx_grid_x(nvec, dev::kMxFoldUnroll<PDCC_V(n)>, 1, dev::kMxGridReduce));
            hipLaunchKernelGGL((dev::k_mx_fold<PDCC_V(f), PDCC_V(dt), PDCC_V(n), PDCC_V(avg), PDCC_V(rot)>), grid, dim3(256), 0,
                               stream, in, c, avg_div, d, numel, signs);
          });
        });
      });
    });
  });
  return hipGetLastError();
}
#undef PDCC_V
}  // namespace

hipError_t mx_quantize(const void* src, size_t numel, DType t, void* wire, size_t cb, size_t nchunks, hipStream_t stream,
                       const MxOpts& opts) {
  MxOpts o = opts;
  if (numel == 0 && !o.sr) o.residual = nullptr;  // (no elements: no residual to update, the wire is all padding blocks)
  if (!mx_args_ok(o, true, cb, wire, numel ? src : nullptr) || !mx_dtype_ok(t) || !mx_chunks_ok(nchunks))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock || !mx_sr_fits(o, numel)) return hipErrorInvalidValue;
  return mx_quantize_launch(MxLayout::DEALT, src, numel, 0, t, wire, cb, nchunks, stream, o);
}

hipError_t mx_quantize_shards(const void* src, size_t m, DType t, void* wire, size_t cb, size_t nchunks,
                              hipStream_t stream, const MxOpts& o) {
  if (!mx_args_ok(o, true, cb, wire, src) || !mx_dtype_ok(t) || !mx_shards_ok(m, cb, nchunks)) return hipErrorInvalidValue;
  if (!mx_sr_fits(o, m * nchunks)) return hipErrorInvalidValue;
  return mx_quantize_launch(mx_shard_layout(m, t), src, m * nchunks, m, t, wire, cb, nchunks, stream, o);
}

hipError_t mx_quantize_list(const MxListTensor* ts, size_t k, DType t, void* wire, size_t cb, size_t nchunks,
                            hipStream_t stream, const MxOpts& o) {
  return mx_list_run<true>(ts, k, t, static_cast<char*>(wire), cb, nchunks, stream, o);
}

hipError_t mx_reduce(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out, hipStream_t stream,
                     const MxOpts& o) {
  if (!mx_args_ok(o, true, cb, wire_in, wire_out) || !mx_fold_ok(nsrc, op, avg_div)) return hipErrorInvalidValue;
  if (o.sr && o.sr->index_offset) return hipErrorInvalidValue;  // (the word index is the element's index in the chunk)
  return mx_reduce_launch(wire_in, nsrc, cb, op, avg_div, wire_out, stream, o);
}

hipError_t mx_dequantize(const void* wire, size_t cb, size_t nchunks, void* dst, size_t numel, DType t,
                         hipStream_t stream, const MxOpts& o) {
  if (!mx_args_ok(o, false, cb, wire, numel ? dst : nullptr) || !mx_dtype_ok(t) || !mx_chunks_ok(nchunks))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  return mx_dequantize_launch(MxLayout::DEALT, wire, cb, nchunks, dst, numel, 0, t, stream, o);
}

hipError_t mx_dequantize_shards(const void* wire, size_t cb, size_t nchunks, void* dst, size_t m, DType t,
                                hipStream_t stream, const MxOpts& o) {
  if (!mx_args_ok(o, false, cb, wire, dst) || !mx_dtype_ok(t) || !mx_shards_ok(m, cb, nchunks)) return hipErrorInvalidValue;
  return mx_dequantize_launch(mx_shard_layout(m, t), wire, cb, nchunks, dst, m * nchunks, m, t, stream, o);
}

hipError_t mx_dequantize_list(const void* wire, size_t cb, size_t nchunks, const MxListTensor* ts, size_t k, DType t,
                              hipStream_t stream, const MxOpts& o) {
  return mx_list_run<false>(ts, k, t, const_cast<char*>(static_cast<const char*>(wire)), cb, nchunks, stream, o);
}

hipError_t mx_fold(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* dst, size_t numel, DType t,
                   hipStream_t stream, const MxOpts& o) {
  if (!mx_args_ok(o, false, cb, wire_in, dst) || !mx_dtype_ok(t) || !mx_fold_ok(nsrc, op, avg_div)) return hipErrorInvalidValue;
  if (numel == 0 || numel > cb * kMxBlock) return hipErrorInvalidValue;
  return mx_fold_launch(wire_in, nsrc, cb, op, avg_div, dst, numel, t, stream, o);
}

}  // namespace kern
}  // namespace pdcc
