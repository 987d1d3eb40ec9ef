// The IPC collectives' protocol table and launch plan: what the host must know about each
// kern::IpcColl, and everything ipc_launch decides before it launches. Header-only, no torch
// header, no HIP runtime call. The comment block on the enum (kernel_api.h) is the prose
// description of the protocols; this table is the machine-readable one, and the single place
// to add a protocol (plus its kernel body).
#pragma once
#include <type_traits>

#include "kernel_api.h"

namespace pdcc {
namespace kern {

enum class ZcUnit : uint8_t { NONE, TILE, ROW };               // what a zero-copy call's bytes are whole multiples of
enum class Staging : uint8_t { NONE, CHUNK, WCHUNKS, ROWS };   // one padded chunk, W of them, whole rows of W tiles
enum class GridBy : uint8_t { TILES, ROWS, LINES, ONE };       // what the picked grid counts (LINES: 8-byte lines)
enum class Family : uint8_t {                                  // the kernel template that runs the protocol
  IPC_COPY, IPC_REDUCE, LL_ALLREDUCE, LL_ALLGATHER, LL_REDUCE, LL_ROOTED, LL_REDUCE_SCATTER, LL_ALLTOALL
};
inline const char* family_name(Family f) {
  constexpr const char* n[] = {"k_ipc_copy", "k_ipc_reduce", "k_ll_allreduce", "k_ll_allgather",
                               "k_ll_reduce", "k_ll_rooted", "k_ll_reduce_scatter", "k_ll_alltoall"};
  return n[(int)f];
}

struct CollTraits {
  IpcColl coll;
  bool ll;          // flag-tagged push protocol (no staging, no barrier; payload <= kLLMaxBytes)
  bool ll_rooted;   // ... that needs a valid root (tokens on the pairs that carry no data)
  bool reducing;    // dispatched on (dtype, op)
  ZcUnit zc_unit;   // NONE: no zero-copy variant
  bool zc_stages;   // a zero-copy call still stages results
  bool zc_only;     // no staged variant
  Staging staging;  // of a staged call
  GridBy grid;
  Family family;
  IpcColl ll_twin;   // the small-payload protocol of the same collective (kCount: none)
  IpcColl one_shot;  // the 1-shot protocol of the same collective (kCount: none)
};

namespace detail {
using C = IpcColl;
using Z = ZcUnit;
using S = Staging;
using G = GridBy;
using F = Family;
constexpr C kNone = C::kCount;
constexpr CollTraits ll_row(C c, bool rooted, bool reducing, F f) {
  return {c, true, rooted, reducing, Z::NONE, false, false, S::NONE, G::LINES, f, kNone, kNone};
}
constexpr CollTraits kCollTraits[] = {
    // coll              ll     rooted reduce zc unit  zc_stg zc_only staging     grid      family         LL twin               1-shot twin
    {C::ALLREDUCE_1SHOT, false, false, true,  Z::NONE, false, false, S::CHUNK,   G::TILES, F::IPC_REDUCE, C::ALLREDUCE_LL,      kNone},
    {C::ALLREDUCE_2SHOT, false, false, true,  Z::ROW,  false, false, S::ROWS,    G::ROWS,  F::IPC_REDUCE, C::ALLREDUCE_LL,      C::ALLREDUCE_1SHOT},
    {C::REDUCE_1SHOT,    false, false, true,  Z::NONE, false, false, S::CHUNK,   G::TILES, F::IPC_REDUCE, C::REDUCE_LL,         kNone},
    {C::REDUCE_2SHOT,    false, false, true,  Z::ROW,  true,  false, S::ROWS,    G::ROWS,  F::IPC_REDUCE, C::REDUCE_LL,         C::REDUCE_1SHOT},
    {C::BROADCAST_1SHOT, false, false, false, Z::NONE, false, false, S::CHUNK,   G::TILES, F::IPC_COPY,   C::BROADCAST_LL,      kNone},
    {C::BROADCAST_2SHOT, false, false, false, Z::ROW,  false, false, S::ROWS,    G::ROWS,  F::IPC_COPY,   C::BROADCAST_LL,      C::BROADCAST_1SHOT},
    {C::ALLGATHER,       false, false, false, Z::TILE, false, false, S::CHUNK,   G::TILES, F::IPC_COPY,   C::ALLGATHER_LL,      kNone},
    {C::GATHER,          false, false, false, Z::TILE, false, false, S::CHUNK,   G::TILES, F::IPC_COPY,   C::GATHER_LL,         kNone},
    {C::SCATTER,         false, false, false, Z::TILE, false, false, S::WCHUNKS, G::TILES, F::IPC_COPY,   C::SCATTER_LL,        kNone},
    {C::REDUCE_SCATTER,  false, false, true,  Z::TILE, false, false, S::WCHUNKS, G::TILES, F::IPC_REDUCE, C::REDUCE_SCATTER_LL, kNone},
    {C::ALLTOALL,        false, false, false, Z::TILE, false, false, S::WCHUNKS, G::TILES, F::IPC_COPY,   C::ALLTOALL_LL,       kNone},
    {C::BARRIER,         false, false, false, Z::NONE, false, false, S::NONE,    G::ONE,   F::IPC_COPY,   kNone,                kNone},
    {C::ALLREDUCE_PUSH,  false, false, true,  Z::ROW,  true,  true,  S::NONE,    G::ROWS,  F::IPC_REDUCE, C::ALLREDUCE_LL,      kNone},
    ll_row(C::ALLREDUCE_LL, false, true, F::LL_ALLREDUCE),
    ll_row(C::ALLGATHER_LL, false, false, F::LL_ALLGATHER),
    ll_row(C::REDUCE_LL, true, true, F::LL_REDUCE),
    ll_row(C::BROADCAST_LL, true, false, F::LL_ROOTED),
    ll_row(C::GATHER_LL, true, false, F::LL_ROOTED),
    ll_row(C::SCATTER_LL, true, false, F::LL_ROOTED),
    ll_row(C::REDUCE_SCATTER_LL, false, true, F::LL_REDUCE_SCATTER),
    ll_row(C::ALLTOALL_LL, false, false, F::LL_ALLTOALL),
};
constexpr int kRows = (int)(sizeof(kCollTraits) / sizeof(kCollTraits[0]));
constexpr bool rows_in_order(int i = 0) {
  return i == kRows || ((int)kCollTraits[i].coll == i && rows_in_order(i + 1));
}
static_assert(kRows == (int)IpcColl::kCount, "one row per protocol");
static_assert(rows_in_order(), "row i describes protocol i");
}  // namespace detail

constexpr const CollTraits& coll_traits(IpcColl c) { return detail::kCollTraits[(int)c]; }
constexpr bool is_ll(IpcColl c) { return coll_traits(c).ll; }
// the protocol that runs `c`'s collective from staging (a zero-copy-only protocol has another one for that)
constexpr IpcColl staged_twin(IpcColl c) { return coll_traits(c).zc_only ? IpcColl::ALLREDUCE_2SHOT : c; }

// bool: SUM == logical OR == MAX, PROD == logical AND == MIN (ProcessGroupNCCL semantics)
inline void canon(DType& t, RedOp& op) {
  if (t == DType::BOOL) {
    t = DType::U8;
    if (op == RedOp::SUM) op = RedOp::MAX;
    if (op == RedOp::PROD) op = RedOp::MIN;
  }
}

constexpr size_t pad_to(size_t n, size_t unit) { return (n + unit - 1) / unit * unit; }

// Bytes of staging needed for `c` (padded to tiles).
inline size_t ipc_staging_bytes(const IpcCall& c, int world) {
  const CollTraits& t = coll_traits(c.coll);
  const size_t cpad = pad_to(c.bytes, kTileBytes);
  // zero-copy: peers read the user buffers in place; a rooted reduce stages its reduced tiles, the
  // push all-reduce receives W slots of bytes / W
  const size_t zc = t.zc_stages ? cpad : 0;
  if (c.zc && !c.gate) return zc;
  size_t staged = 0;
  switch (coll_traits(c.gate ? staged_twin(c.coll) : c.coll).staging) {
    case Staging::NONE: break;  // flags only, straight into LL slots, or zero-copy only (rejected by ipc_plan)
    case Staging::CHUNK: staged = cpad; break;
    case Staging::WCHUNKS: staged = cpad * world; break;
    // whole rows of W tiles: phase 2 (dev::OwnerRowMap) reads a partial last row's padding
    case Staging::ROWS: staged = pad_to(cpad, (size_t)world * kTileBytes); break;
  }
  return c.gate && zc > staged ? zc : staged;  // a gated call may run either protocol: the larger need
}

// What ipc_launch does with `c` in a group of `world` ranks: reject it (`err`), or launch `family`
// (for `world`, and for the reducing ones the canonical `dtype` and `op`) on `grid` workgroups. The
// grid is part of the protocol: a function of the call's arguments only, identical on every rank.
struct IpcPlan {
  hipError_t err;
  int grid;
  Family family;
  DType dtype;
  RedOp op;
};

inline IpcPlan ipc_plan(int world, const IpcCall& c) {
  IpcPlan p{hipErrorInvalidValue, 0, Family::IPC_COPY, c.dtype, c.op};
  if (world < 2 || world > kMaxRanks) return p;
  const CollTraits& t = coll_traits(c.coll);
  p.family = t.family;
  if (c.gate && (c.zc || t.ll)) return p;  // the kernel picks zc for a gated call
  if (c.zc || c.gate) {  // in-place reads of user buffers: whole tiles (2-shot: whole rows of W tiles), no over-read
    const size_t unit = (size_t)kTileBytes * (t.zc_unit == ZcUnit::ROW ? world : 1);
    if (t.zc_unit == ZcUnit::NONE || c.bytes == 0 || c.bytes % unit != 0) return p;
  } else if (t.zc_only) {
    return p;
  }
  if (t.ll && (c.zc || c.bytes == 0 || c.bytes > kLLMaxBytes)) return p;
  if (t.ll_rooted && (c.root < 0 || c.root >= world)) return p;
  if (t.reducing) {
    if (!supports(c.dtype, c.op) || c.op == RedOp::COPY) return p;
    canon(p.dtype, p.op);
  }
  const size_t nt = (c.bytes + kTileBytes - 1) / kTileBytes;
  const size_t cap = c.grid_cap > 0 ? (size_t)c.grid_cap : 0;
  size_t grid = c.grid > 0 ? (size_t)c.grid : 0;
  if (!grid) {
    switch (t.grid) {
      case GridBy::TILES: grid = nt; break;
      case GridBy::ROWS: grid = (nt + world - 1) / world; break;
      case GridBy::LINES: grid = ((c.bytes + 7) / 8 + kBlockThreads - 1) / kBlockThreads; break;  // one line per thread
      case GridBy::ONE: grid = 1; break;
    }
    const size_t hi = cap ? cap : 512;
    grid = grid < 1 ? 1 : grid > hi ? hi : grid;
  }
  if (cap && grid > cap) grid = cap;
  if (grid > (size_t)kMaxBlocks) grid = kMaxBlocks;
  // a gated zero-copy launch with the device-side exchange: one more workgroup, block 0, does only
  // the exchange (dev::xchg_blocks); the data blocks keep the grid every rank computes the same way
  if (c.gate && c.ztab) grid = (grid < (size_t)kMaxBlocks - 1 ? grid : (size_t)kMaxBlocks - 1) + 1;
  p.grid = (int)grid;
  p.err = hipSuccess;
  return p;
}

// f(std::integral_constant<int, W>{}) for the group's world size W (2 .. kMaxRanks)
template <class Fn>
hipError_t by_world(int w, Fn&& f) {
  switch (w) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kern
}  // namespace pdcc
