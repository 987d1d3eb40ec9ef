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
//
// The wire variants (WF below) also write the block-scaled wire of the rounded new master, which saves the quantizer
// its launch and the 2 + 2 bytes per bf16 element of the round trip through param_out: a 32-element block is the
// eight adjacent lanes of one round, the lane layout of the f32 k_mx_quantize, so the block amax is the same DPP
// butterfly and the payload stores are the same accesses (mx_fmt.h). No LDS, no scratch
// (profiles/zero/adamw_wire_resources.txt).
#include <algorithm>

#include "group_io.h"
#include "mx_fmt.h"

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

// GD: the gradient's dtype. PD: the parameter dtype, param_out's; HASP = false: no param_out (PD unused).
// WF: kNoWire, or the MxFormat of the wire the same pass emits ("Parameter wire from the step"): the new master
// rounded once to PD and widened again is quantized as group gi = i / 4 of a one-chunk wire of `cbw` blocks (mx_emit4:
// the block amax over the eight lanes that hold the block, the format's scale, pack<4> and store). The loop then runs
// over all 8 cbw groups of the wire, whole waves: a group past numel loads and stores nothing of the tensors and emits
// zeros, so the blank tail blocks get payload 0 and scale byte 127. Vector path only; param_out is stored when given.
template <DType GD, DType PD, bool HASP, bool VEC, int WF = kNoWire>
__global__ __launch_bounds__(256) void k_adamw(const char* grad, char* master, char* exp_avg, char* exp_avg_sq,
                                               char* param_out, size_t numel, const kern::AdamWArgs a,
                                               const double* __restrict__ total, float max_norm, char* wire,
                                               size_t cbw) {
#pragma clang fp contract(off)
  using G = typename Tr<GD>::S;
  using P = typename Tr<PD>::S;
  constexpr DType F = DType::F32;
  constexpr bool WIRE = WF != kNoWire;
  static_assert(!WIRE || (VEC && HASP), "the wire variants: vector path, PD always meaningful");
  const bool sp = HASP && (!WIRE || param_out != nullptr);
  const float coef = total ? clip_coef(total, max_norm) : 1.0f;
  const size_t ngroups = WIRE ? cbw * (kern::kMxBlock / kE) : (numel + kE - 1) / kE;
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
      const size_t gi = g0 + (size_t)u * 256 + threadIdx.x, i = gi * kE;
#pragma unroll
      for (int j = 0; j < kE; ++j) adamw_elem(g[u][j] * coef, m[u][j], v[u][j], p[u][j], a);
      if (VEC && i + kE <= numel) {
        store_group<F, kE, kNtState>(master + i * 4, p[u]);
        store_group<F, kE, kNtState>(exp_avg + i * 4, m[u]);
        store_group<F, kE, kNtState>(exp_avg_sq + i * 4, v[u]);
        if constexpr (HASP) {
          if (sp) store_group<PD, kE>(param_out + i * sizeof(P), p[u]);
        }
      } else {
        store_elems<F, kE>(master, i, numel, p[u]);
        store_elems<F, kE>(exp_avg, i, numel, m[u]);
        store_elems<F, kE>(exp_avg_sq, i, numel, v[u]);
        if constexpr (HASP) {
          if (sp) store_elems<PD, kE>(param_out, i, numel, p[u]);
        }
      }
      if constexpr (WIRE) {
        if (gi < ngroups) {  // (the same for a whole wave: 8 cbw is a multiple of 128)
          float r[kE];
#pragma unroll
          for (int j = 0; j < kE; ++j) r[j] = i + j < numel ? round_as<PD>(p[u][j]) : 0.0f;
          mx_emit4<(kern::MxFormat)WF>(wire, cbw, gi, r);
        }
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
  void* wire;
  size_t cbw;
};

template <DType GD, DType PD>
bool adamw_vec(const Launch& l, bool hasp) {
  return aligned(l.grad, kE * sizeof(typename Tr<GD>::S)) && aligned(l.master, 16) && aligned(l.exp_avg, 16) &&
         aligned(l.exp_avg_sq, 16) && (!hasp || aligned(l.param_out, kE * sizeof(typename Tr<PD>::S)));
}
template <class K>
hipError_t adamw_launch(K k, const Launch& l) {
  hipLaunchKernelGGL(k, dim3(l.grid), dim3(256), 0, l.stream, (const char*)l.grad, (char*)l.master, (char*)l.exp_avg,
                     (char*)l.exp_avg_sq, (char*)l.param_out, l.numel, *l.a, l.total, l.max_norm, (char*)l.wire, l.cbw);
  return hipGetLastError();
}

template <DType GD, DType PD, bool HASP>
hipError_t adamw_go(const Launch& l) {
  return adamw_launch(adamw_vec<GD, PD>(l, HASP) ? k_adamw<GD, PD, HASP, true> : k_adamw<GD, PD, HASP, false>, l);
}

template <DType GD>
hipError_t adamw_pick(const Launch& l, DType pt) {
  if (!l.param_out) return adamw_go<GD, DType::F32, false>(l);
  if (pt == DType::F32) return adamw_go<GD, DType::F32, true>(l);
  return adamw_go<GD, GD, true>(l);
}

// the wire variants: the vector path or nothing
template <DType GD, DType PD>
hipError_t adamw_wire_go(const Launch& l, kern::MxFormat f) {
  if (!adamw_vec<GD, PD>(l, l.param_out != nullptr) || !aligned(l.wire, 16)) return hipErrorInvalidValue;
  switch (f) {
    case kern::MxFormat::FP8_E4M3: return adamw_launch(k_adamw<GD, PD, true, true, (int)kern::MxFormat::FP8_E4M3>, l);
    case kern::MxFormat::FP4_E2M1: return adamw_launch(k_adamw<GD, PD, true, true, (int)kern::MxFormat::FP4_E2M1>, l);
    default: return adamw_launch(k_adamw<GD, PD, true, true, (int)kern::MxFormat::FP6_E2M3>, l);
  }
}
template <DType GD>
hipError_t adamw_wire_pick(const Launch& l, const kern::AdamWWire& w) {
  if constexpr (GD != DType::F32) {
    if (w.dt == GD) return adamw_wire_go<GD, GD>(l, w.fmt);
  }
  return adamw_wire_go<GD, DType::F32>(l, w.fmt);
}

}  // namespace
}  // namespace dev

namespace kern {

// sixteen workgroups per CU, four of them resident at the kernels' 4 waves per SIMD: a workgroup's sixteen loads per
// lane are in flight while the others compute and store
constexpr int kAdamWGrid = 4096;

hipError_t adamw_step(const void* grad, DType gt, float* master, float* exp_avg, float* exp_avg_sq, void* param_out,
                      DType pt, size_t numel, const AdamWArgs& a, const double* total, float max_norm,
                      hipStream_t stream, int max_blocks, const AdamWWire& wire) {
  if (gt != DType::F32 && gt != DType::BF16 && gt != DType::F16) return hipErrorInvalidValue;
  if (param_out && pt != DType::F32 && pt != gt) return hipErrorInvalidValue;
  if (wire.out && ((wire.dt != DType::F32 && wire.dt != gt) || (param_out && pt != wire.dt))) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  if (!grad || !master || !exp_avg || !exp_avg_sq) return hipErrorInvalidValue;
  const size_t cap = max_blocks > 0 ? (size_t)max_blocks : (size_t)kAdamWGrid;
  const size_t cbw = wire.out ? mx_chunk_blocks(wire.fmt, numel, 1) : 0;
  const size_t covered = wire.out ? cbw * kMxBlock : numel;  // the wire's blank tail blocks too
  const int grid = (int)std::min<size_t>((covered + kAdamWSpan - 1) / kAdamWSpan, cap);
  const dev::Launch l{grad, master, exp_avg, exp_avg_sq, param_out, numel, &a, total, max_norm, grid, stream, wire.out, cbw};
  if (wire.out) {
    switch (gt) {
      case DType::F32: return dev::adamw_wire_pick<DType::F32>(l, wire);
      case DType::BF16: return dev::adamw_wire_pick<DType::BF16>(l, wire);
      default: return dev::adamw_wire_pick<DType::F16>(l, wire);
    }
  }
  switch (gt) {
    case DType::F32: return dev::adamw_pick<DType::F32>(l, pt);
    case DType::BF16: return dev::adamw_pick<DType::BF16>(l, pt);
    default: return dev::adamw_pick<DType::F16>(l, pt);
  }
}

}  // namespace kern
}  // namespace pdcc
