// Fused AdamW step on a ZeRO shard (docs/collectives.md "Fused AdamW step"): what ShardedOptimizer(params,
// "adamw") runs between the last bucket wait and the parameter all-gather, in place of clip_scale, the inner
// optimizer's step and the master -> param_shard cast. One pass, 28 bytes per element for bf16 parameters:
//
//   read   grad (2 or 4 B, once: non-temporal), master, exp_avg, exp_avg_sq (f32)
//   write  master, exp_avg, exp_avg_sq (f32, in place) and, with param_out, the new master rounded once
//
// k_adamw. Every lane reads the f64 total (a uniform address: one scalar load per wave) and evaluates the clip
// coefficient as k_clip_scale does, or takes 1 without a total. Then a grid-strided stream over groups of four
// elements: 16 bytes on every f32 side, 8 bytes on a 16-bit side. Group j of a trip goes to lane j % 256 in
// round j / 256, so a wave's accesses of one round are 1 KiB contiguous per f32 stream. A lane issues the loads
// of all four streams for its kAdamWUnroll = 4 groups (16 vector loads in flight, 64 VGPRs of payload), and only
// then computes and stores group by group: it reads all of its groups before it writes any and touches no other
// lane's, so the update is in place. The arithmetic is f32 with contraction off, in the documented order, so
// the plain-PyTorch reference rounds where the kernel rounds. A base that is not vector-aligned on any side takes
// the element path (VEC = false: the same groups, one element at a time); the group that straddles numel is
// masked element by element in both. Nothing at or past numel is read or written.
//
// The state stores are non-temporal (the state is next read a whole training step later): next to plain stores, two
// builds alternating in one run, the bf16 step at a 64 MiB shard took 156-160 us instead of 182-183, the f32 step at
// 64 MiB and both at 1 GiB stayed within 0.7 %. PDCC_ADAMW_NT_STATE=0 at compile time brings the plain
// stores back. param_out is always a plain store: the all-gather or the wire's quantizer reads it next.
#include <algorithm>

#include "group_io.h"

#ifndef PDCC_ADAMW_NT_STATE
#define PDCC_ADAMW_NT_STATE 1
#endif

namespace pdcc {
namespace dev {

namespace {

constexpr int kE = 4;  // elements of a group
constexpr int kU = kern::kAdamWUnroll;
constexpr bool kNtState = PDCC_ADAMW_NT_STATE != 0;
static_assert(kern::kAdamWSpan == (size_t)kern::kBlockThreads * kU * kE, "a trip is 256 lanes x kU groups");

// one element: the five steps of the contract, every operation rounded to f32 on its own
__device__ __forceinline__ void adamw_elem(float g, float& m, float& v, float& p, const kern::AdamWArgs& a) {
#pragma clang fp contract(off)
  m = a.beta1 * m + a.one_minus_beta1 * g;
  v = a.beta2 * v + a.one_minus_beta2 * (g * g);
  p = p * a.decay;
  p = p - a.step_size * (m / (sqrtf(v) * a.inv_sqrt_bc2 + a.eps));
}

// GD: the gradient's dtype. PD: param_out's; HASP = false: no param_out (PD unused)
template <DType GD, DType PD, bool HASP, bool VEC>
__global__ __launch_bounds__(256) void k_adamw(const char* grad, char* master, char* exp_avg, char* exp_avg_sq,
                                               char* param_out, size_t numel, const kern::AdamWArgs a,
                                               const double* __restrict__ total, float max_norm) {
#pragma clang fp contract(off)
  using G = typename Tr<GD>::S;
  using P = typename Tr<PD>::S;
  constexpr DType F = DType::F32;
  const float coef = total ? clip_coef(total, max_norm) : 1.0f;
  const size_t ngroups = (numel + kE - 1) / kE;
  for (size_t g0 = (size_t)blockIdx.x * (256 * kU); g0 < ngroups; g0 += (size_t)gridDim.x * (256 * kU)) {
    float g[kU][kE], p[kU][kE], m[kU][kE], v[kU][kE];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const size_t i = (g0 + (size_t)u * 256 + threadIdx.x) * kE;
      if (VEC && i + kE <= numel) {
        load_group<GD, kE>(grad + i * sizeof(G), g[u]);
        load_group<F, kE, false>(master + i * 4, p[u]);
        load_group<F, kE, false>(exp_avg + i * 4, m[u]);
        load_group<F, kE, false>(exp_avg_sq + i * 4, v[u]);
      } else {  // (a group wholly past the end reads nothing: +0 everywhere, and stores nothing below)
        load_elems<GD, kE>(grad, i, numel, g[u]);
        load_elems<F, kE>(master, i, numel, p[u]);
        load_elems<F, kE>(exp_avg, i, numel, m[u]);
        load_elems<F, kE>(exp_avg_sq, i, numel, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const size_t i = (g0 + (size_t)u * 256 + threadIdx.x) * kE;
#pragma unroll
      for (int j = 0; j < kE; ++j) adamw_elem(g[u][j] * coef, m[u][j], v[u][j], p[u][j], a);
      if (VEC && i + kE <= numel) {
        store_group<F, kE, kNtState>(master + i * 4, p[u]);
        store_group<F, kE, kNtState>(exp_avg + i * 4, m[u]);
        store_group<F, kE, kNtState>(exp_avg_sq + i * 4, v[u]);
        if constexpr (HASP) store_group<PD, kE>(param_out + i * sizeof(P), p[u]);
      } else {
        store_elems<F, kE>(master, i, numel, p[u]);
        store_elems<F, kE>(exp_avg, i, numel, m[u]);
        store_elems<F, kE>(exp_avg_sq, i, numel, v[u]);
        if constexpr (HASP) store_elems<PD, kE>(param_out, i, numel, p[u]);
      }
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

struct Launch {
  const void* grad;
  float *master, *exp_avg, *exp_avg_sq;
  void* param_out;
  size_t numel;
  const kern::AdamWArgs* a;
  const double* total;
  float max_norm;
  int grid;
  hipStream_t stream;
};

template <DType GD, DType PD, bool HASP>
hipError_t adamw_go(const Launch& l) {
  const bool vec = aligned(l.grad, kE * sizeof(typename Tr<GD>::S)) && aligned(l.master, 16) &&
                   aligned(l.exp_avg, 16) && aligned(l.exp_avg_sq, 16) &&
                   (!HASP || aligned(l.param_out, kE * sizeof(typename Tr<PD>::S)));
  auto k = vec ? k_adamw<GD, PD, HASP, true> : k_adamw<GD, PD, HASP, false>;
  hipLaunchKernelGGL(k, dim3(l.grid), dim3(256), 0, l.stream, (const char*)l.grad, (char*)l.master, (char*)l.exp_avg,
                     (char*)l.exp_avg_sq, (char*)l.param_out, l.numel, *l.a, l.total, l.max_norm);
  return hipGetLastError();
}

template <DType GD>
hipError_t adamw_pick(const Launch& l, DType pt) {
  if (!l.param_out) return adamw_go<GD, DType::F32, false>(l);
  if (pt == DType::F32) return adamw_go<GD, DType::F32, true>(l);
  return adamw_go<GD, GD, true>(l);
}

}  // namespace
}  // namespace dev

namespace kern {

// sixteen workgroups per CU, four of them resident at the kernels' 4 waves per SIMD: a workgroup's sixteen loads per
// lane are in flight while the others compute and store
constexpr int kAdamWGrid = 4096;

hipError_t adamw_step(const void* grad, DType gt, float* master, float* exp_avg, float* exp_avg_sq, void* param_out,
                      DType pt, size_t numel, const AdamWArgs& a, const double* total, float max_norm,
                      hipStream_t stream, int max_blocks) {
  if (gt != DType::F32 && gt != DType::BF16 && gt != DType::F16) return hipErrorInvalidValue;
  if (param_out && pt != DType::F32 && pt != gt) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  if (!grad || !master || !exp_avg || !exp_avg_sq) return hipErrorInvalidValue;
  const size_t cap = max_blocks > 0 ? (size_t)max_blocks : (size_t)kAdamWGrid;
  const int grid = (int)std::min<size_t>((numel + kAdamWSpan - 1) / kAdamWSpan, cap);
  const dev::Launch l{grad, master, exp_avg, exp_avg_sq, param_out, numel, &a, total, max_norm, grid, stream};
  switch (gt) {
    case DType::F32: return dev::adamw_pick<DType::F32>(l, pt);
    case DType::BF16: return dev::adamw_pick<DType::BF16>(l, pt);
    default: return dev::adamw_pick<DType::F16>(l, pt);
  }
}

}  // namespace kern
}  // namespace pdcc
