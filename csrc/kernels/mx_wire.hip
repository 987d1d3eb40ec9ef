// The local kernels of the block-scaled FP8 wire format `mxfp8_e4m3` (layout: mx_layout.h,
// contract: docs/collectives.md "Compressed all-reduce" and "Compressed reduce-scatter and
// all-gather"):
//
//   mx_quantize    f32 / bf16 / f16 tensor -> wire           (reads 4n or 2n, writes 33n/32)
//   mx_reduce      nsrc chunk wires -> one chunk wire         (dequantize, fold in f32, requantize)
//   mx_dequantize  wire -> f32 / bf16 / f16 tensor
//   mx_fold        nsrc chunk wires -> f32 / bf16 / f16 tensor (dequantize, fold in f32, round once)
//   mx_quantize_shards / mx_dequantize_shards: quantize / dequantize with one chunk per shard of m
//                  elements (the SHARD instantiations of the same two kernels)
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
#include <algorithm>

#include "dev_common.h"
#include "mx_layout.h"

namespace pdcc {
namespace dev {

namespace {

using F8 = Tr<DType::F8E4M3>;
constexpr int kMxUnroll = 4;  // independent 16-B loads in flight per lane (quantize / dequantize)

// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror: lane ^ 1, lane ^ 2, 7 - lane (of 8)
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t x) {
  const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
  return x > y ? x : y;
}
// max over the LANES (2, 4 or 8) aligned neighbours that share a block; every one of them is active
template <int LANES>
__device__ __forceinline__ uint32_t group_max(uint32_t x) {
  x = dpp_max<kDppXor1>(x);
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

// ---------------------------------------------------------------------------- quantize
// Lane layout of one chunk (grid row): vector v of the chunk is 16 B of the tensor = EPL elements,
// LPB = 32 / EPL consecutive lanes make a block. The chunk has cb * LPB vectors, a multiple of 64.
// SHARD: chunk r is the `m` elements from r * m on (numel = nchunks * m) instead of the 32 cb from
// r * 32 cb on, and nothing at or past (r + 1) * m enters it. VEC = false (shards that do not start
// 16-byte aligned) reads every element on its own.
template <DType DT, bool SHARD, bool VEC>
__global__ __launch_bounds__(256) void k_mx_quantize(const char* __restrict__ src, size_t numel,
                                                     char* __restrict__ wire, uint32_t cb, size_t m) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  const size_t chunk = blockIdx.y;
  char* __restrict__ w = wire + chunk * kern::mx_chunk_bytes(cb);
  const size_t el0 = SHARD ? chunk * m : chunk * cb * (size_t)kern::kMxBlock;  // first element of the chunk
  const size_t end = SHARD ? el0 + m : numel;                                  // one past its last
  const uint32_t nvec = cb * LPB;
  // a workgroup takes one contiguous span of kMxUnroll * 256 vectors per pass (16 KiB of the tensor)
  constexpr uint32_t stride = 256u;
  const uint32_t pass = gridDim.x * 256u * kMxUnroll;
  for (uint32_t v0 = blockIdx.x * 256u * kMxUnroll + threadIdx.x; v0 < nvec; v0 += pass) {
    S s[kMxUnroll][EPL];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      const size_t el = el0 + (size_t)v * EPL;
      if (VEC && v < nvec && el + EPL <= end) {
        const uint4 x = *reinterpret_cast<const uint4*>(src + el * sizeof(S));
        __builtin_memcpy(s[u], &x, 16);
      } else {
        // the last vector, or padding: elements past the end count as +0 and are never read
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
          S z;
          __builtin_memset(&z, 0, sizeof(S));
          if (v < nvec && el + i < end) z = reinterpret_cast<const S*>(src)[el + i];
          s[u][i] = z;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      if (v >= nvec) break;  // (whole waves leave together: nvec and every span start are multiples of 64)
      float f[EPL];
      uint32_t am = 0;
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        f[i] = T::in(s[u][i]);
        const uint32_t a = abs_bits(f[i]);
        am = a > am ? a : am;
      }
      const MxScale sc = mx_scale(group_max<LPB>(am));
      uint32_t q[EPL / 4];
#pragma unroll
      for (int d = 0; d < EPL / 4; ++d) {
        q[d] = narrow4(f[4 * d], f[4 * d + 1], f[4 * d + 2], f[4 * d + 3], sc.inv);
        if (sc.blank) q[d] = 0u;
      }
      char* p = w + (size_t)v * EPL;  // payload byte e of the chunk is element e of the chunk
      if constexpr (EPL == 4) *reinterpret_cast<uint32_t*>(p) = q[0];
      else *reinterpret_cast<uint2*>(p) = make_uint2(q[0], q[1]);
      if (v % LPB == 0) w[kern::mx_scale_off(cb, v / LPB)] = (char)sc.byte;
    }
  }
}

// ---------------------------------------------------------------------------- dequantize
// The same lane layout as quantize: a lane reads EPL payload bytes and its block's scale byte and
// stores 16 B of the tensor; nothing at or past `numel` is written. SHARD / VEC as in quantize:
// chunk r fills exactly dst[r m, (r + 1) m).
template <DType DT, bool SHARD, bool VEC>
__global__ __launch_bounds__(256) void k_mx_dequantize(const char* __restrict__ wire, uint32_t cb,
                                                       char* __restrict__ dst, size_t numel, size_t m) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  const size_t chunk = blockIdx.y;
  const char* __restrict__ w = wire + chunk * kern::mx_chunk_bytes(cb);
  const size_t el0 = SHARD ? chunk * m : chunk * cb * (size_t)kern::kMxBlock;
  if (el0 >= numel) return;  // a padding chunk
  const size_t left = SHARD ? m : numel - el0;
  // vectors of this chunk that hold at least one element of the tensor
  const uint32_t nvec = (uint32_t)(left >= (size_t)cb * kern::kMxBlock ? (size_t)cb * LPB : (left + EPL - 1) / EPL);
  constexpr uint32_t stride = 256u;  // (contiguous spans per workgroup, as in quantize)
  const uint32_t pass = gridDim.x * 256u * kMxUnroll;
  for (uint32_t v0 = blockIdx.x * 256u * kMxUnroll + threadIdx.x; v0 < nvec; v0 += pass) {
    uint32_t q[kMxUnroll][EPL / 4];
    uint32_t sb[kMxUnroll];
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      sb[u] = 127u;
#pragma unroll
      for (int d = 0; d < EPL / 4; ++d) q[u][d] = 0u;
      if (v < nvec) {
        const char* p = w + (size_t)v * EPL;
        if constexpr (EPL == 4) {
          q[u][0] = *reinterpret_cast<const uint32_t*>(p);
        } else {
          const uint2 x = *reinterpret_cast<const uint2*>(p);
          q[u][0] = x.x;
          q[u][1] = x.y;
        }
        sb[u] = (uint8_t)w[kern::mx_scale_off(cb, v / LPB)];
      }
    }
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      const uint32_t v = v0 + u * stride;
      if (v >= nvec) break;
      const float scale = mx_scale_value(sb[u]);
      float f[EPL];
#pragma unroll
      for (int d = 0; d < EPL / 4; ++d) widen4(q[u][d], scale, f + 4 * d);
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
// A lane takes 16 payload bytes (half a block) of every source, so a block is two neighbouring
// lanes and the amax of the folded block is one exchange between them.
template <int NSRC, bool AVG>
__global__ __launch_bounds__(256) void k_mx_reduce(const char* __restrict__ in, uint32_t cb, int avg_div,
                                                   char* __restrict__ out) {
  const size_t cbytes = kern::mx_chunk_bytes(cb);
  const uint32_t nvec = cb * 2u;
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nvec; v += stride) {
    uint4 p[NSRC];
    uint32_t sb[NSRC];
#pragma unroll
    for (int r = 0; r < NSRC; ++r) {
      const char* c = in + (size_t)r * cbytes;
      p[r] = *reinterpret_cast<const uint4*>(c + (size_t)v * 16);
      sb[r] = (uint8_t)c[kern::mx_scale_off(cb, v >> 1)];
    }
    float acc[16];
#pragma unroll
    for (int r = 0; r < NSRC; ++r) {
      const float scale = mx_scale_value(sb[r]);
      const uint32_t w[4] = {p[r].x, p[r].y, p[r].z, p[r].w};
      float f[16];
#pragma unroll
      for (int d = 0; d < 4; ++d) widen4(w[d], scale, f + 4 * d);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = r == 0 ? f[i] : acc[i] + f[i];  // rank order
    }
    if constexpr (AVG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = acc[i] / (float)avg_div;
    }
    uint32_t am = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t a = abs_bits(acc[i]);
      am = a > am ? a : am;
    }
    const MxScale sc = mx_scale(group_max<2>(am));
    uint32_t q[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      q[d] = narrow4(acc[4 * d], acc[4 * d + 1], acc[4 * d + 2], acc[4 * d + 3], sc.inv);
      if (sc.blank) q[d] = 0u;
    }
    *reinterpret_cast<uint4*>(out + (size_t)v * 16) = make_uint4(q[0], q[1], q[2], q[3]);
    if ((v & 1u) == 0) out[kern::mx_scale_off(cb, v >> 1)] = (char)sc.byte;
  }
}

// ---------------------------------------------------------------------------- fold
// nsrc chunk wires -> a tensor: what mx_reduce then mx_dequantize would give without the wire in
// between (and without its requantization). The lane layout is dequantize's: the wide side is the
// output, 16 B = EPL elements per lane, so a lane reads EPL payload bytes and its block's scale byte
// of every source and a wave's store is contiguous. All NSRC * U loads are issued before the first
// convert; U keeps about eight of them in flight per lane whatever NSRC is.
template <int NSRC>
constexpr int kMxFoldUnroll = NSRC <= 2 ? 4 : (NSRC <= 4 ? 2 : 1);

template <DType DT, int NSRC, bool AVG>
__global__ __launch_bounds__(256) void k_mx_fold(const char* __restrict__ in, uint32_t cb, int avg_div,
                                                 char* __restrict__ dst, size_t numel) {
  using T = Tr<DT>;
  using S = typename T::S;
  constexpr int EPL = 16 / (int)sizeof(S);
  constexpr int LPB = kern::kMxBlock / EPL;
  constexpr int U = kMxFoldUnroll<NSRC>;
  const size_t cbytes = kern::mx_chunk_bytes(cb);
  const uint32_t nvec = (uint32_t)((numel + EPL - 1) / EPL);  // <= cb * LPB: numel <= 32 cb
  const uint32_t pass = gridDim.x * 256u * U;
  for (uint32_t v0 = blockIdx.x * 256u * U + threadIdx.x; v0 < nvec; v0 += pass) {
    uint32_t q[U][NSRC][EPL / 4];
    uint32_t sb[U][NSRC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t v = v0 + u * 256u;
#pragma unroll
      for (int r = 0; r < NSRC; ++r) {
        sb[u][r] = 127u;
#pragma unroll
        for (int d = 0; d < EPL / 4; ++d) q[u][r][d] = 0u;
        if (v < nvec) {
          const char* c = in + (size_t)r * cbytes;
          const char* p = c + (size_t)v * EPL;
          if constexpr (EPL == 4) {
            q[u][r][0] = *reinterpret_cast<const uint32_t*>(p);
          } else {
            const uint2 x = *reinterpret_cast<const uint2*>(p);
            q[u][r][0] = x.x;
            q[u][r][1] = x.y;
          }
          sb[u][r] = (uint8_t)c[kern::mx_scale_off(cb, v / LPB)];
        }
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
#pragma unroll
        for (int d = 0; d < EPL / 4; ++d) widen4(q[u][r][d], scale, f + 4 * d);
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = r == 0 ? f[i] : acc[i] + f[i];  // source order
      }
      if constexpr (AVG) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = acc[i] / (float)avg_div;
      }
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
}  // namespace

hipError_t mx_quantize(const void* src, size_t numel, DType t, void* wire, size_t cb, size_t nchunks,
                       hipStream_t stream) {
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(src)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock) return hipErrorInvalidValue;
  const int lpb = t == DType::F32 ? 8 : 4;
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
  const char* s = static_cast<const char*>(src);
  char* w = static_cast<char*>(wire);
  switch (t) {
    case DType::F32: hipLaunchKernelGGL((dev::k_mx_quantize<DType::F32, false, true>), grid, dim3(256), 0, stream, s, numel, w, (uint32_t)cb, size_t(0)); break;
    case DType::BF16: hipLaunchKernelGGL((dev::k_mx_quantize<DType::BF16, false, true>), grid, dim3(256), 0, stream, s, numel, w, (uint32_t)cb, size_t(0)); break;
    case DType::F16: hipLaunchKernelGGL((dev::k_mx_quantize<DType::F16, false, true>), grid, dim3(256), 0, stream, s, numel, w, (uint32_t)cb, size_t(0)); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t mx_dequantize(const void* wire, size_t cb, size_t nchunks, void* dst, size_t numel, DType t,
                         hipStream_t stream) {
  if (!mx_cb_ok(cb) || nchunks == 0 || nchunks > 65535 || !mx_al16(wire) || (numel && !mx_al16(dst)))
    return hipErrorInvalidValue;
  if (numel > cb * nchunks * kMxBlock) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  const int lpb = t == DType::F32 ? 8 : 4;
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
  const char* w = static_cast<const char*>(wire);
  char* d = static_cast<char*>(dst);
  switch (t) {
    case DType::F32: hipLaunchKernelGGL((dev::k_mx_dequantize<DType::F32, false, true>), grid, dim3(256), 0, stream, w, (uint32_t)cb, d, numel, size_t(0)); break;
    case DType::BF16: hipLaunchKernelGGL((dev::k_mx_dequantize<DType::BF16, false, true>), grid, dim3(256), 0, stream, w, (uint32_t)cb, d, numel, size_t(0)); break;
    case DType::F16: hipLaunchKernelGGL((dev::k_mx_dequantize<DType::F16, false, true>), grid, dim3(256), 0, stream, w, (uint32_t)cb, d, numel, size_t(0)); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

namespace {
size_t mx_esize(DType t) { return t == DType::F32 ? 4 : 2; }
// the shard arguments: m elements per shard fit the chunk, and the whole tensor's size is a size_t
bool mx_shards_ok(size_t m, size_t cb, size_t nchunks) {
  return mx_cb_ok(cb) && m > 0 && m <= cb * kMxBlock && nchunks > 0 && nchunks <= 65535;
}

template <DType DT>
void mx_quantize_shards_go(const dim3& grid, bool vec, const char* s, size_t numel, char* w, uint32_t cb, size_t m,
                           hipStream_t stream) {
  if (vec) hipLaunchKernelGGL((dev::k_mx_quantize<DT, true, true>), grid, dim3(256), 0, stream, s, numel, w, cb, m);
  else hipLaunchKernelGGL((dev::k_mx_quantize<DT, true, false>), grid, dim3(256), 0, stream, s, numel, w, cb, m);
}
template <DType DT>
void mx_dequantize_shards_go(const dim3& grid, bool vec, const char* w, uint32_t cb, char* d, size_t numel, size_t m,
                             hipStream_t stream) {
  if (vec) hipLaunchKernelGGL((dev::k_mx_dequantize<DT, true, true>), grid, dim3(256), 0, stream, w, cb, d, numel, m);
  else hipLaunchKernelGGL((dev::k_mx_dequantize<DT, true, false>), grid, dim3(256), 0, stream, w, cb, d, numel, m);
}
}  // namespace

hipError_t mx_quantize_shards(const void* src, size_t m, DType t, void* wire, size_t cb, size_t nchunks,
                              hipStream_t stream) {
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(src)) return hipErrorInvalidValue;
  if (t != DType::F32 && t != DType::BF16 && t != DType::F16) return hipErrorInvalidValue;
  const int lpb = t == DType::F32 ? 8 : 4;
  const bool vec = m * mx_esize(t) % 16 == 0;  // every shard starts 16-byte aligned
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
  const char* s = static_cast<const char*>(src);
  char* w = static_cast<char*>(wire);
  const size_t numel = m * nchunks;
  switch (t) {
    case DType::F32: mx_quantize_shards_go<DType::F32>(grid, vec, s, numel, w, (uint32_t)cb, m, stream); break;
    case DType::BF16: mx_quantize_shards_go<DType::BF16>(grid, vec, s, numel, w, (uint32_t)cb, m, stream); break;
    default: mx_quantize_shards_go<DType::F16>(grid, vec, s, numel, w, (uint32_t)cb, m, stream); break;
  }
  return hipGetLastError();
}

hipError_t mx_dequantize_shards(const void* wire, size_t cb, size_t nchunks, void* dst, size_t m, DType t,
                                hipStream_t stream) {
  if (!mx_shards_ok(m, cb, nchunks) || !mx_al16(wire) || !mx_al16(dst)) return hipErrorInvalidValue;
  if (t != DType::F32 && t != DType::BF16 && t != DType::F16) return hipErrorInvalidValue;
  const int lpb = t == DType::F32 ? 8 : 4;
  const bool vec = m * mx_esize(t) % 16 == 0;
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * lpb, dev::kMxUnroll, nchunks, dev::kMxGridStream), (uint32_t)nchunks);
  const char* w = static_cast<const char*>(wire);
  char* d = static_cast<char*>(dst);
  const size_t numel = m * nchunks;
  switch (t) {
    case DType::F32: mx_dequantize_shards_go<DType::F32>(grid, vec, w, (uint32_t)cb, d, numel, m, stream); break;
    case DType::BF16: mx_dequantize_shards_go<DType::BF16>(grid, vec, w, (uint32_t)cb, d, numel, m, stream); break;
    default: mx_dequantize_shards_go<DType::F16>(grid, vec, w, (uint32_t)cb, d, numel, m, stream); break;
  }
  return hipGetLastError();
}

namespace {
template <bool AVG>
hipError_t mx_reduce_go(const char* in, int nsrc, uint32_t cb, int avg_div, char* out, hipStream_t stream) {
  const dim3 grid(dev::mx_grid_x((uint64_t)cb * 2, 1, 1, dev::kMxGridReduce)), block(256);
  switch (nsrc) {
#define PDCC_MX_N(N) \
  case N: hipLaunchKernelGGL((dev::k_mx_reduce<N, AVG>), grid, block, 0, stream, in, cb, avg_div, out); break;
    PDCC_MX_N(1) PDCC_MX_N(2) PDCC_MX_N(3) PDCC_MX_N(4) PDCC_MX_N(5) PDCC_MX_N(6) PDCC_MX_N(7) PDCC_MX_N(8)
#undef PDCC_MX_N
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
}  // namespace

hipError_t mx_reduce(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* wire_out,
                     hipStream_t stream) {
  if (!mx_cb_ok(cb) || nsrc < 1 || nsrc > kMaxRanks || !mx_al16(wire_in) || !mx_al16(wire_out))
    return hipErrorInvalidValue;
  if (op != RedOp::SUM && op != RedOp::AVG) return hipErrorInvalidValue;
  if (op == RedOp::AVG && avg_div < 1) return hipErrorInvalidValue;
  const char* in = static_cast<const char*>(wire_in);
  char* out = static_cast<char*>(wire_out);
  return op == RedOp::AVG ? mx_reduce_go<true>(in, nsrc, (uint32_t)cb, avg_div, out, stream)
                          : mx_reduce_go<false>(in, nsrc, (uint32_t)cb, avg_div, out, stream);
}

namespace {
template <DType DT, bool AVG>
hipError_t mx_fold_go(const char* in, int nsrc, uint32_t cb, int avg_div, char* dst, size_t numel, hipStream_t stream) {
  constexpr int epl = 16 / (int)sizeof(typename dev::Tr<DT>::S);
  const uint64_t nvec = (numel + epl - 1) / epl;
  const dim3 block(256);
  switch (nsrc) {
#define PDCC_MX_N(N)                                                                                        \
  case N: {                                                                                                 \
    const dim3 grid(dev::mx_grid_x(nvec, dev::kMxFoldUnroll<N>, 1, dev::kMxGridReduce));                    \
    hipLaunchKernelGGL((dev::k_mx_fold<DT, N, AVG>), grid, block, 0, stream, in, cb, avg_div, dst, numel); \
    break;                                                                                                  \
  }
    PDCC_MX_N(1) PDCC_MX_N(2) PDCC_MX_N(3) PDCC_MX_N(4) PDCC_MX_N(5) PDCC_MX_N(6) PDCC_MX_N(7) PDCC_MX_N(8)
#undef PDCC_MX_N
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <DType DT>
hipError_t mx_fold_op(const char* in, int nsrc, uint32_t cb, RedOp op, int avg_div, char* dst, size_t numel,
                      hipStream_t stream) {
  return op == RedOp::AVG ? mx_fold_go<DT, true>(in, nsrc, cb, avg_div, dst, numel, stream)
                          : mx_fold_go<DT, false>(in, nsrc, cb, avg_div, dst, numel, stream);
}
}  // namespace

hipError_t mx_fold(const void* wire_in, int nsrc, size_t cb, RedOp op, int avg_div, void* dst, size_t numel, DType t,
                   hipStream_t stream) {
  if (!mx_cb_ok(cb) || nsrc < 1 || nsrc > kMaxRanks || !mx_al16(wire_in) || !mx_al16(dst))
    return hipErrorInvalidValue;
  if (numel == 0 || numel > cb * kMxBlock) return hipErrorInvalidValue;
  if (op != RedOp::SUM && op != RedOp::AVG) return hipErrorInvalidValue;
  if (op == RedOp::AVG && avg_div < 1) return hipErrorInvalidValue;
  const char* in = static_cast<const char*>(wire_in);
  char* d = static_cast<char*>(dst);
  switch (t) {
    case DType::F32: return mx_fold_op<DType::F32>(in, nsrc, (uint32_t)cb, op, avg_div, d, numel, stream);
    case DType::BF16: return mx_fold_op<DType::BF16>(in, nsrc, (uint32_t)cb, op, avg_div, d, numel, stream);
    case DType::F16: return mx_fold_op<DType::F16>(in, nsrc, (uint32_t)cb, op, avg_div, d, numel, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kern
}  // namespace pdcc
