// Gradient clipping by global norm (docs/collectives.md "Gradient clipping"): the two kernels
// ShardedOptimizer(max_grad_norm=...) runs between the last bucket wait and the inner optimizer's step.
//
//   sumsq       the sum of the squares of a list of f32 / bf16 / f16 tensors as one f64, the same bits for
//               any grid and any base alignment: two plain launches, no atomics, no last-block counter
//   clip_scale  out[i] = round_once((float)src[i] * coef), coef = min(1, max_norm / (sqrt(total) + 1e-6))
//               computed on the device from the f64 total -- the host never sees the norm
//
// sumsq, stage 1 (k_sumsq_tiles, one launch per tensor). The tensor is cut into tiles of kSumsqTile = 8192
// elements counted from its element 0; a workgroup of 256 lanes takes whole tiles, grid-strided, and writes
// one f64 per tile to partials[tile]. Inside a tile the elements are dealt in groups of E = 16 bytes' worth
// (4 f32, 8 bf16 / f16): group j goes to lane j % 256 in round j / 256, so a wave's loads of one round are
// 1 KiB contiguous. A lane issues the 16-byte non-temporal loads of all its rounds (8 for f32, 4 for the
// 16-bit types), widens to f32 and runs ONE chain acc = fmaf(x, x, acc) from +0 over its 32 elements, rounds
// in order and elements in index order: 32 roundings. The 64 lane values of a wave are folded by a fixed DPP
// tree (lane ^ 1, lane ^ 2, row_half_mirror, row_mirror, row_bcast:15, row_bcast:31; lane 63 holds the sum):
// 6 more f32 roundings. So no f32 chain from an element to its tile partial is longer than
//
//     L = kSumsqChain = 32 + 6 = 38 roundings.
//
// The four wave sums cross LDS as they are and are added in f64, (w0 + w1) + (w2 + w3); everything from there
// on is f64. Which lane holds which element depends on the dtype and on nothing else: a base pointer that is
// not 16-byte aligned takes the element path (VEC = false: the same groups, loaded one element at a time),
// and the last, partial tile loads its straddling group element by element and counts what lies past the
// end as +0 -- fmaf(0, 0, acc) is acc. Nothing at or past src + numel is read.
//
// sumsq, stage 2 (k_sumsq_fold, one workgroup). Lane l adds partials l, l + 256, ... in order in f64 (eight
// loads in flight, added in index order), the 256 lane values go through one fixed LDS tree (stride 128, 64,
// .., 1), lane 0 writes the f64. The partials of all tensors are concatenated in list order.
//
// clip_scale (k_clip_scale). Every lane reads the total (a uniform address: one scalar load per wave) and
// evaluates torch's formula in f32; NaN stays NaN. Then a grid-strided stream, four independent groups per
// lane in flight: a group is 16 bytes on the wider of the two sides (4 elements when either side is f32, 8
// for bf16 -> bf16 / f16 -> f16), loaded non-temporally (read once), multiplied in f32, rounded once to the
// output dtype and stored as one vector. A lane reads its groups before it writes them and touches no other
// lane's, so out may be src. Misaligned bases (either side) take the element path; the group that straddles
// the end is masked element by element in both.
#include <algorithm>

#include "group_io.h"

namespace pdcc {
namespace dev {

namespace {

constexpr int kT = kern::kSumsqTile;
static_assert(kT == kern::kBlockThreads * 32 && kern::kSumsqChain == 32 + 6, "a lane's chain is 32 elements");

// x + (the DPP-selected lane's x); rows the mask leaves out add +0
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dpp_add(float x) {
  const float y = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), CTRL, ROWS, 0xf, false));
  return x + y;
}
// The fixed tree of a wave64: after the first four steps every lane of a row of 16 holds the row's sum, then
// rows 1 and 3 add the row before them and rows 2, 3 add row 1: lane 63 holds the wave's sum.
__device__ __forceinline__ float wave_sum_lane63(float x) {
  x = dpp_add<0xB1>(x);        // quad_perm [1,0,3,2]: lane ^ 1
  x = dpp_add<0x4E>(x);        // quad_perm [2,3,0,1]: lane ^ 2
  x = dpp_add<0x141>(x);       // row_half_mirror: the other quad of the eight
  x = dpp_add<0x140>(x);       // row_mirror: the other eight of the row
  x = dpp_add<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
  x = dpp_add<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3
  return x;
}

template <DType DT, bool VEC>
__global__ __launch_bounds__(256) void k_sumsq_tiles(const char* __restrict__ src, size_t numel,
                                                     double* __restrict__ partials) {
  using S = typename Tr<DT>::S;
  constexpr int E = 16 / (int)sizeof(S);  // elements of a group
  constexpr int R = kT / (256 * E);       // rounds of a tile
  __shared__ float wsum[2][4];            // by the tile's parity: one barrier per tile
  const uint32_t lane = threadIdx.x;
  const size_t ntiles = (numel + kT - 1) / kT;
  uint32_t par = 0;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    const size_t e0 = tile * kT;
    float f[R][E];
    if (VEC && e0 + kT <= numel) {
#pragma unroll
      for (int r = 0; r < R; ++r) load_group<DT, E>(src + (e0 + (size_t)(r * 256 + lane) * E) * sizeof(S), f[r]);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const size_t i = e0 + (size_t)(r * 256 + lane) * E;
        if (VEC && i + E <= numel) load_group<DT, E>(src + i * sizeof(S), f[r]);
        else load_elems<DT, E>(src, i, numel, f[r]);
      }
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < E; ++j) acc = fmaf(f[r][j], f[r][j], acc);
    acc = wave_sum_lane63(acc);
    if ((lane & 63u) == 63u) wsum[par][lane >> 6] = acc;
    __syncthreads();
    if (lane == 0)
      partials[tile] = ((double)wsum[par][0] + (double)wsum[par][1]) + ((double)wsum[par][2] + (double)wsum[par][3]);
  }
}

__global__ __launch_bounds__(256) void k_sumsq_fold(const double* __restrict__ partials, size_t n,
                                                    double* __restrict__ out) {
  __shared__ double s[256];
  const uint32_t lane = threadIdx.x;
  double acc = 0.0;
  size_t i = lane;
  for (; i + 7 * 256 < n; i += 8 * 256) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = partials[i + k * 256];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  for (; i < n; i += 256) acc += partials[i];
  s[lane] = acc;
  __syncthreads();
  for (uint32_t h = 128; h >= 1; h >>= 1) {
    if (lane < h) s[lane] += s[lane + h];
    __syncthreads();
  }
  if (lane == 0) out[0] = s[0];
}

constexpr int kClipUnroll = 4;  // independent groups in flight per lane

template <DType SD, DType OD, bool VEC>
__global__ __launch_bounds__(256) void k_clip_scale(const char* src, const double* __restrict__ total, float max_norm,
                                                    char* out, size_t numel) {
  using S = typename Tr<SD>::S;
  using O = typename Tr<OD>::S;
  constexpr int E = 16 / (int)(sizeof(S) > sizeof(O) ? sizeof(S) : sizeof(O));
  constexpr int U = kClipUnroll;
  const float coef = clip_coef(total, max_norm);
  const size_t ngroups = (numel + E - 1) / E;
  for (size_t g0 = (size_t)blockIdx.x * (256 * U); g0 < ngroups; g0 += (size_t)gridDim.x * (256 * U)) {
    float f[U][E];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = (g0 + (size_t)u * 256 + threadIdx.x) * E;
      if (VEC && i + E <= numel) load_group<SD, E>(src + i * sizeof(S), f[u]);
      else load_elems<SD, E>(src, i, numel, f[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = (g0 + (size_t)u * 256 + threadIdx.x) * E;
#pragma unroll
      for (int j = 0; j < E; ++j) f[u][j] *= coef;
      if (VEC && i + E <= numel) store_group<OD, E>(out + i * sizeof(O), f[u]);
      else store_elems<OD, E>(out, i, numel, f[u]);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <DType DT>
hipError_t sumsq_go(const void* src, size_t numel, double* partials, int grid, hipStream_t stream) {
  if (aligned16(src))
    hipLaunchKernelGGL((k_sumsq_tiles<DT, true>), dim3(grid), dim3(256), 0, stream, (const char*)src, numel, partials);
  else
    hipLaunchKernelGGL((k_sumsq_tiles<DT, false>), dim3(grid), dim3(256), 0, stream, (const char*)src, numel, partials);
  return hipGetLastError();
}

template <DType SD, DType OD>
hipError_t clip_go(const void* src, const double* total, float max_norm, void* out, size_t numel, int grid,
                   hipStream_t stream) {
  if (aligned16(src) && aligned16(out))
    hipLaunchKernelGGL((k_clip_scale<SD, OD, true>), dim3(grid), dim3(256), 0, stream, (const char*)src, total, max_norm,
                       (char*)out, numel);
  else
    hipLaunchKernelGGL((k_clip_scale<SD, OD, false>), dim3(grid), dim3(256), 0, stream, (const char*)src, total, max_norm,
                       (char*)out, numel);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

namespace kern {

// eight workgroups per CU hide a tile's load latency behind the other tiles' fold
constexpr int kClipGrid = 2048;

hipError_t sumsq(const SumsqTensor* ts, size_t k, double* partials, double* out, hipStream_t stream, int max_blocks) {
  if (!partials || !out || (k && !ts)) return hipErrorInvalidValue;
  size_t at = 0;
  for (size_t i = 0; i < k; ++i) {
    const SumsqTensor& t = ts[i];
    if (t.numel == 0) continue;
    if (!t.ptr) return hipErrorInvalidValue;
    const size_t tiles = sumsq_tiles(t.numel);
    const int grid = (int)std::min<size_t>(tiles, max_blocks > 0 ? (size_t)max_blocks : (size_t)kClipGrid);
    hipError_t e;
    switch (t.t) {
      case DType::F32: e = dev::sumsq_go<DType::F32>(t.ptr, t.numel, partials + at, grid, stream); break;
      case DType::BF16: e = dev::sumsq_go<DType::BF16>(t.ptr, t.numel, partials + at, grid, stream); break;
      case DType::F16: e = dev::sumsq_go<DType::F16>(t.ptr, t.numel, partials + at, grid, stream); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    at += tiles;
  }
  hipLaunchKernelGGL(dev::k_sumsq_fold, dim3(1), dim3(256), 0, stream, (const double*)partials, at, out);
  return hipGetLastError();
}

hipError_t clip_scale(const void* src, DType st, const double* total, float max_norm, void* out, DType ot, size_t numel,
                      hipStream_t stream) {
  if (ot != DType::F32 && ot != st) return hipErrorInvalidValue;
  if (st != DType::F32 && st != DType::BF16 && st != DType::F16) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  if (!src || !out || !total) return hipErrorInvalidValue;
  const size_t e = 16 / std::max(dtype_size(st), dtype_size(ot));
  const size_t per_block = (size_t)kBlockThreads * dev::kClipUnroll * e;
  const int grid = (int)std::min<size_t>((numel + per_block - 1) / per_block, (size_t)kClipGrid);
  using namespace dev;
  if (st == DType::F32) return clip_go<DType::F32, DType::F32>(src, total, max_norm, out, numel, grid, stream);
  if (st == DType::BF16)
    return ot == DType::F32 ? clip_go<DType::BF16, DType::F32>(src, total, max_norm, out, numel, grid, stream)
                            : clip_go<DType::BF16, DType::BF16>(src, total, max_norm, out, numel, grid, stream);
  return ot == DType::F32 ? clip_go<DType::F16, DType::F32>(src, total, max_norm, out, numel, grid, stream)
                          : clip_go<DType::F16, DType::F16>(src, total, max_norm, out, numel, grid, stream);
}

}  // namespace kern
}  // namespace pdcc
