// Fused AdamW step on a ZeRO shard with block-scaled 8-bit state (docs/collectives.md "8-bit AdamW state"): what
// ShardedOptimizer(params, "adamw", state_format="mxfp8_e4m3") runs in place of k_adamw (adamw.hip). exp_avg and the
// square root of exp_avg_sq are each one dealt `mxfp8_e4m3` wire of one chunk (mx_layout.h):
// [32 cb payload bytes][cb scale bytes], cb = mx_chunk_blocks(numel, 1), block b = elements 32 b .. 32 b + 31. One
// pass, 16.1 bytes per element for bf16 parameters (20.1 for f32) instead of 28 (32):
//
//   read   grad (2 or 4 B, once: non-temporal), master (4), one payload byte of each moment (2), the two scale bytes
//          of the block (2 / 32)
//   write  master (4), the two payload bytes (2), the two scale bytes (2 / 32) and, with param_out, the new master
//          rounded once (2 or 4)
//
// k_adamw8 keeps k_adamw's work split: groups of four elements, 256 lanes, kAdamWUnroll groups per lane, group j of a
// trip on lane j % 256 in round j / 256, 4096 elements per workgroup and trip. A 32-element block is therefore the
// eight adjacent lanes of one round. The loop runs over whole blocks: all eight lanes of a block that starts before
// numel are active, the groups past numel load nothing, count as +0 and store zero codes (the payload area holds
// whole blocks: cb >= the number of blocks). Per group a lane loads the gradient, the master, one payload dword of each
// moment (four e4m3 codes) and the block's two scale bytes, widens with the packed FP8 converts, and after the update
// requantizes: the block amax of each moment is a DPP butterfly over the eight lanes on the f32 bits (group_max<8>),
// the scale comes from mx_scale_of, the payload from narrow4 (mx_block.h: the wire quantizer's rule, so exp_avg is byte
// for byte ops.mx_quantize_reference of the new m). The second moment is stored as s = sqrtf(v), and a positive s is
// never stored as code 0: its scaled value is raised to 2^-9, the smallest e4m3 subnormal, before the convert. The
// master and param_out come from the unquantized m and s of this step.
//
// In place. A lane reads all of its groups before it writes any and its payload dwords and master belong to it alone.
// A block's scale byte is read by the block's eight lanes and written by the first of them: the eight sit in one wave
// (a wave is 64 consecutive lanes of a round, a block never spans two), a wave issues all loads of a trip before its
// first store, and the stored byte depends on every one of those loads through the butterfly. No other wave touches
// the block. The state buffers are 16-byte aligned, always; grad, master and param_out that are not vector-aligned
// take the element path (VEC = false), the same bits. The master's stores are non-temporal as in k_adamw; the payload
// and scale stores are plain (not measured either way). No LDS, no scratch (profiles/zero/adamw8_resources.txt).
#include <algorithm>

#include "group_io.h"
#include "mx_block.h"
#include "mx_fmt.h"
#include "mx_layout.h"

#ifndef PDCC_ADAMW_NT_STATE
#define PDCC_ADAMW_NT_STATE 1
#endif

namespace pdcc {
namespace dev {

namespace {

constexpr int kE = 4;  // elements of a group
constexpr int kU = kern::kAdamWUnroll;
constexpr int kLanes = kern::kMxBlock / kE;  // lanes of a block
constexpr bool kNtMaster = PDCC_ADAMW_NT_STATE != 0;
static_assert(kern::kAdamWSpan == (size_t)kern::kBlockThreads * kU * kE, "a trip is 256 lanes x kU groups");
static_assert(kLanes == 8 && 256 % kLanes == 0, "a block is eight adjacent lanes of one round");

// the scale of a block of e4m3 codes (largest magnitude 448 = 1.75 2^8; mx_wire.hip MxFmt<FP8_E4M3>::scale)
__device__ __forceinline__ MxScale scale8(uint32_t amax) { return mx_scale_of<8, 0x600000u, -117, 120>(amax); }

// GD: the gradient's dtype. PD: the parameter dtype, param_out's; HASP = false: no param_out (PD unused). exp_avg /
// exp_avg_sqrt: the state wires, chunks of cb blocks; the tensors hold the span that starts at block `block0` of them
// (0, with cb = mx_chunk_blocks(numel, 1): the whole shard), so the span's payload starts at byte 32 block0 and its
// scale bytes at 32 cb + block0.
// WF: kNoWire, or the MxFormat of the parameter wire the same pass emits, as in k_adamw (adamw.hip): the loop then
// runs over the 8 cbw groups of that wire (cbw >= the span's blocks, and no relation to cb), the groups past the span's
// blocks touch nothing of the state and emit zeros. Vector path only; param_out is stored when given.
template <DType GD, DType PD, bool HASP, bool VEC, int WF = kNoWire>
__global__ __launch_bounds__(256) void k_adamw8(const char* grad, char* master, char* exp_avg, char* exp_avg_sqrt,
                                                char* param_out, size_t numel, size_t cb, size_t block0,
                                                const kern::AdamWArgs a, const double* __restrict__ total,
                                                float max_norm, char* wire, size_t cbw) {
#pragma clang fp contract(off)
  using G = typename Tr<GD>::S;
  using P = typename Tr<PD>::S;
  constexpr DType F = DType::F32;
  constexpr bool WIRE = WF != kNoWire;
  static_assert(!WIRE || (VEC && HASP), "the wire variants: vector path, PD always meaningful");
  const bool sp = HASP && (!WIRE || param_out != nullptr);
  const float coef = total ? clip_coef(total, max_norm) : 1.0f;
  const size_t ngroups = kern::mx_blocks(numel) * kLanes;  // whole blocks
  const size_t nloop = WIRE ? cbw * kLanes : ngroups;
  const size_t scales = kern::mx_scale_off(cb, block0) - kern::mx_payload_off(block0);  // from the span's payload
  exp_avg += kern::mx_payload_off(block0);
  exp_avg_sqrt += kern::mx_payload_off(block0);
  for (size_t g0 = (size_t)blockIdx.x * (256 * kU); g0 < nloop; g0 += (size_t)gridDim.x * (256 * kU)) {
    float g[kU][kE], p[kU][kE];
    uint32_t qm[kU], qs[kU], em[kU], es[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const size_t gi = g0 + (size_t)u * 256 + threadIdx.x, i = gi * kE;
      if (VEC && i + kE <= numel) {
        load_group<GD, kE>(grad + i * sizeof(G), g[u]);
        load_group<F, kE, false>(master + i * 4, p[u]);
      } else {  // (a group wholly past the end reads nothing: +0 everywhere)
        load_elems<GD, kE>(grad, i, numel, g[u]);
        load_elems<F, kE>(master, i, numel, p[u]);
      }
      qm[u] = qs[u] = 0u, em[u] = es[u] = 127u;
      if (gi < ngroups) {  // (the same for the eight lanes of a block)
        qm[u] = *reinterpret_cast<const uint32_t*>(exp_avg + i);
        qs[u] = *reinterpret_cast<const uint32_t*>(exp_avg_sqrt + i);
        em[u] = *reinterpret_cast<const uint8_t*>(exp_avg + scales + gi / kLanes);
        es[u] = *reinterpret_cast<const uint8_t*>(exp_avg_sqrt + scales + gi / kLanes);
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const size_t gi = g0 + (size_t)u * 256 + threadIdx.x, i = gi * kE;
      if (gi < ngroups) {
        float m[kE], s[kE];
        widen4(qm[u], mx_scale_value(em[u]), m);
        widen4(qs[u], mx_scale_value(es[u]), s);
        uint32_t am = 0u, as = 0u;
#pragma unroll
        for (int j = 0; j < kE; ++j) {
          if (i + j >= numel) m[j] = s[j] = 0.0f;  // positions past the end count as +0, whatever the buffer holds
          const float gj = g[u][j] * coef;
          const float v0 = s[j] * s[j];
          m[j] = a.beta1 * m[j] + a.one_minus_beta1 * gj;
          const float v = a.beta2 * v0 + a.one_minus_beta2 * (gj * gj);
          p[u][j] = p[u][j] * a.decay;
          s[j] = sqrtf(v);
          p[u][j] = p[u][j] - a.step_size * (m[j] / (s[j] * a.inv_sqrt_bc2 + a.eps));
          const uint32_t bm = abs_bits(m[j]), bs = abs_bits(s[j]);
          am = bm > am ? bm : am;
          as = bs > as ? bs : as;
        }
        const MxScale sm = scale8(group_max<kLanes>(am)), ss = scale8(group_max<kLanes>(as));
#pragma unroll
        for (int j = 0; j < kE; ++j) {  // a positive s is stored as at least the smallest subnormal
          const float t = s[j] * ss.inv;
          s[j] = (s[j] > 0.0f && t < 0.001953125f) ? 0.001953125f : t;
        }
        const uint32_t wm = sm.blank ? 0u : narrow4(m[0], m[1], m[2], m[3], sm.inv);
        const uint32_t ws = ss.blank ? 0u : narrow4(s[0], s[1], s[2], s[3], 1.0f);
        *reinterpret_cast<uint32_t*>(exp_avg + i) = wm;
        *reinterpret_cast<uint32_t*>(exp_avg_sqrt + i) = ws;
        if ((threadIdx.x & (kLanes - 1)) == 0) {
          *reinterpret_cast<uint8_t*>(exp_avg + scales + gi / kLanes) = (uint8_t)sm.byte;
          *reinterpret_cast<uint8_t*>(exp_avg_sqrt + scales + gi / kLanes) = (uint8_t)ss.byte;
        }
        if (VEC && i + kE <= numel) {
          store_group<F, kE, kNtMaster>(master + i * 4, p[u]);
          if constexpr (HASP) {
            if (sp) store_group<PD, kE>(param_out + i * sizeof(P), p[u]);
          }
        } else {
          store_elems<F, kE>(master, i, numel, p[u]);
          if constexpr (HASP) {
            if (sp) store_elems<PD, kE>(param_out, i, numel, p[u]);
          }
        }
      }
      if constexpr (WIRE) {
        if (gi < nloop) {  // (the same for a whole wave: 8 cbw is a multiple of 128)
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
  float* master;
  uint8_t *exp_avg, *exp_avg_sqrt;
  void* param_out;
  size_t numel, cb, block0;
  const kern::AdamWArgs* a;
  const double* total;
  float max_norm;
  int grid;
  hipStream_t stream;
  void* wire;
  size_t cbw;
};

template <DType GD, DType PD>
bool adamw8_vec(const Launch& l, bool hasp) {
  return aligned(l.grad, kE * sizeof(typename Tr<GD>::S)) && aligned(l.master, 16) &&
         (!hasp || aligned(l.param_out, kE * sizeof(typename Tr<PD>::S)));
}
template <class K>
hipError_t adamw8_launch(K k, const Launch& l) {
  hipLaunchKernelGGL(k, dim3(l.grid), dim3(256), 0, l.stream, (const char*)l.grad, (char*)l.master, (char*)l.exp_avg,
                     (char*)l.exp_avg_sqrt, (char*)l.param_out, l.numel, l.cb, l.block0, *l.a, l.total, l.max_norm,
                     (char*)l.wire, l.cbw);
  return hipGetLastError();
}

template <DType GD, DType PD, bool HASP>
hipError_t adamw8_go(const Launch& l) {
  return adamw8_launch(adamw8_vec<GD, PD>(l, HASP) ? k_adamw8<GD, PD, HASP, true> : k_adamw8<GD, PD, HASP, false>, l);
}

template <DType GD>
hipError_t adamw8_pick(const Launch& l, DType pt) {
  if (!l.param_out) return adamw8_go<GD, DType::F32, false>(l);
  if (pt == DType::F32) return adamw8_go<GD, DType::F32, true>(l);
  return adamw8_go<GD, GD, true>(l);
}

// the wire variants: the vector path or nothing
template <DType GD, DType PD>
hipError_t adamw8_wire_go(const Launch& l, kern::MxFormat f) {
  if (!adamw8_vec<GD, PD>(l, l.param_out != nullptr) || !aligned(l.wire, 16)) return hipErrorInvalidValue;
  switch (f) {
    case kern::MxFormat::FP8_E4M3: return adamw8_launch(k_adamw8<GD, PD, true, true, (int)kern::MxFormat::FP8_E4M3>, l);
    case kern::MxFormat::FP4_E2M1: return adamw8_launch(k_adamw8<GD, PD, true, true, (int)kern::MxFormat::FP4_E2M1>, l);
    default: return adamw8_launch(k_adamw8<GD, PD, true, true, (int)kern::MxFormat::FP6_E2M3>, l);
  }
}
template <DType GD>
hipError_t adamw8_wire_pick(const Launch& l, const kern::AdamWWire& w) {
  if constexpr (GD != DType::F32) {
    if (w.dt == GD) return adamw8_wire_go<GD, GD>(l, w.fmt);
  }
  return adamw8_wire_go<GD, DType::F32>(l, w.fmt);
}

}  // namespace
}  // namespace dev

namespace kern {

constexpr int kAdamW8Grid = 4096;  // as k_adamw's

hipError_t adamw8_step(const void* grad, DType gt, float* master, uint8_t* exp_avg, uint8_t* exp_avg_sqrt,
                       void* param_out, DType pt, size_t numel, const AdamWArgs& a, const double* total,
                       float max_norm, hipStream_t stream, int max_blocks, const AdamWWire& wire, size_t block0,
                       size_t state_cb) {
  if (gt != DType::F32 && gt != DType::BF16 && gt != DType::F16) return hipErrorInvalidValue;
  if (param_out && pt != DType::F32 && pt != gt) return hipErrorInvalidValue;
  if (wire.out && ((wire.dt != DType::F32 && wire.dt != gt) || (param_out && pt != wire.dt))) return hipErrorInvalidValue;
  if (state_cb ? (numel % kMxBlock != 0 || block0 + numel / kMxBlock > state_cb) : block0 != 0) return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  if (!grad || !master || !exp_avg || !exp_avg_sqrt) return hipErrorInvalidValue;
  if (!dev::aligned(exp_avg, 16) || !dev::aligned(exp_avg_sqrt, 16)) return hipErrorInvalidValue;
  const size_t cap = max_blocks > 0 ? (size_t)max_blocks : (size_t)kAdamW8Grid;
  const size_t cbw = wire.out ? mx_chunk_blocks(wire.fmt, numel, 1) : 0;
  const size_t covered = (wire.out ? cbw : mx_blocks(numel)) * kMxBlock;  // whole blocks; the wire's blank tail too
  const int grid = (int)std::min<size_t>((covered + kAdamWSpan - 1) / kAdamWSpan, cap);
  const dev::Launch l{grad, master, exp_avg, exp_avg_sqrt, param_out, numel, state_cb ? state_cb : mx_chunk_blocks(numel, 1),
                      block0, &a, total, max_norm, grid, stream, wire.out, cbw};
  if (wire.out) {
    switch (gt) {
      case DType::F32: return dev::adamw8_wire_pick<DType::F32>(l, wire);
      case DType::BF16: return dev::adamw8_wire_pick<DType::BF16>(l, wire);
      default: return dev::adamw8_wire_pick<DType::F16>(l, wire);
    }
  }
  switch (gt) {
    case DType::F32: return dev::adamw8_pick<DType::F32>(l, pt);
    case DType::BF16: return dev::adamw8_pick<DType::BF16>(l, pt);
    default: return dev::adamw8_pick<DType::F16>(l, pt);
  }
}

}  // namespace kern
}  // namespace pdcc
