// Prints what kern::ipc_plan and kern::ipc_staging_bytes decide for a fixed set of calls, one
// line per call (tests/test_ipc_plan.py compares the lines with tests/golden/ipc_plan.json, which
// was recorded from the launch code as it was before the plan existed). Host only: no GPU, no
// HIP runtime call. Built with ASan + UBSan.
#include <cstdio>
#include <string>

#include "kernels/ipc_plan.h"

using namespace pdcc::kern;

static const char* const kColl[] = {
    "ALLREDUCE_1SHOT", "ALLREDUCE_2SHOT", "REDUCE_1SHOT", "REDUCE_2SHOT", "BROADCAST_1SHOT", "BROADCAST_2SHOT",
    "ALLGATHER", "GATHER", "SCATTER", "REDUCE_SCATTER", "ALLTOALL", "BARRIER", "ALLREDUCE_PUSH", "ALLREDUCE_LL",
    "ALLGATHER_LL", "REDUCE_LL", "BROADCAST_LL", "GATHER_LL", "SCATTER_LL", "REDUCE_SCATTER_LL", "ALLTOALL_LL"};
static const char* const kDType[] = {"F32", "F16", "BF16", "F64", "I8", "U8", "I32", "I64", "BOOL"};
static const char* const kOp[] = {"SUM", "AVG", "PROD", "MIN", "MAX", "BAND", "BOR", "BXOR", "COPY"};
static const char* const kMode[] = {"staged", "zc", "gated", "gated+ztab"};
constexpr int kColls = (int)IpcColl::kCount, kDTypes = (int)DType::kCount, kOps = (int)RedOp::kCount;
static_assert(sizeof(kColl) / sizeof(kColl[0]) == kColls && sizeof(kDType) / sizeof(kDType[0]) == kDTypes &&
                  sizeof(kOp) / sizeof(kOp[0]) == kOps, "a name per enum value");

// the decisions for one call, as text
static std::string decide(int world, const IpcCall& c) {
  const IpcPlan p = ipc_plan(world, c);
  char b[160];
  if (p.err != hipSuccess)
    snprintf(b, sizeof b, "err=%d staging=%zu", (int)p.err, ipc_staging_bytes(c, world));
  else
    snprintf(b, sizeof b, "err=0 grid=%d %s %s %s staging=%zu", p.grid, family_name(p.family), kDType[(int)p.dtype],
             kOp[(int)p.op], ipc_staging_bytes(c, world));
  return b;
}

static void row(int coll, int world, int mode, size_t bytes, int grid = 0, int cap = 0, int root = 0,
                int dtype = (int)DType::F32, int op = (int)RedOp::SUM) {
  static const GateSlot slot{};  // (never read: a gated call is one whose `gate` is set)
  static const ZcTable tab{};
  IpcCall c{};
  c.coll = (IpcColl)coll;
  c.dtype = (DType)dtype;
  c.op = (RedOp)op;
  c.root = root;
  c.avg_div = world;
  c.grid = grid;
  c.grid_cap = cap;
  c.zc = mode == 1;
  c.bytes = bytes;
  c.gate = mode >= 2 ? &slot : nullptr;
  c.ztab = mode == 3 ? &tab : nullptr;
  printf("%s w=%d %s bytes=%zu grid=%d cap=%d root=%d %s %s -> %s\n", kColl[coll], world, kMode[mode], bytes, grid,
         cap, root, kDType[dtype], kOp[op], decide(world, c).c_str());
}

int main() {
  const size_t T = kTileBytes;
  for (int coll = 0; coll < kColls; ++coll)  // every protocol x world x mode x size
    for (int w : {2, 3, 8})
      for (int mode = 0; mode < 4; ++mode)
        for (size_t bytes : {(size_t)0, (size_t)1, (size_t)8, T - 1, T, T + 1, w * T, (w + 1) * T, 3 * w * T + 1028,
                             kLLMaxBytes, kLLMaxBytes + 1, (size_t)64 << 20})
          row(coll, w, mode, bytes);
  for (int coll = 0; coll < kColls; ++coll)  // explicit grids and caps (W = 4)
    for (int mode = 0; mode < 2; ++mode)
      for (size_t bytes : {4 * T, kLLMaxBytes})
        for (int grid : {0, 7, 5000})
          for (int cap : {0, 128}) row(coll, 4, mode, bytes, grid, cap);
  for (int coll = 0; coll < kColls; ++coll)  // roots in and out of range (W = 4)
    for (int root : {-1, 0, 3, 4}) row(coll, 4, 0, 4 * T, 0, 0, root);
  for (int coll : {(int)IpcColl::ALLREDUCE_1SHOT, (int)IpcColl::ALLREDUCE_LL})  // every (dtype, op)
    for (int dt = 0; dt < kDTypes; ++dt)
      for (int op = 0; op < kOps; ++op) row(coll, 4, 0, 4 * T, 0, 0, 0, dt, op);
  for (int w : {1, 9}) row((int)IpcColl::ALLREDUCE_1SHOT, w, 0, T);  // no kernel for these worlds
  return 0;
}
